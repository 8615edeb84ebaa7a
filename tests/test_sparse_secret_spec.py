"""tests/sparse_secret_spec.py, the numpy specification of troyn_sample_ternary_sparse, against the oracle's generator (no GPU needed)."""
import math

import numpy as np
import pytest

import bootstrap_spec as B
import chebyshev_spec as C
import ckks_encode_spec as E
import sparse_secret_spec as S

# the encapsulated bootstrap of tests/test_gpu_sparse_secret_api.py: ephemeral weight, and the EvalMod pair test_the_choice_of_degree_and_double_angles derives
EPHEMERAL_WEIGHT = 32
ENCAPSULATED_DEGREE, ENCAPSULATED_DOUBLE_ANGLES = 39, 2

Q = [1152921504606830593, 1125899906826241, 1099511480321]       # three odd moduli of different sizes; only q - 1 is used


def test_word_order_is_the_centred_binomial_samplers(O):
    """the spec's reader of the block stream re-derives Rng.centered_binomial from the same words: same blocks, same word of each block per coefficient"""
    for n, counter in ((64, 0), (1024, 5)):
        w, after = S.words(O, 0xABCDEF, 7, counter, n)
        ref = O.Rng(0xABCDEF, 7)
        for _ in range(counter):
            ref.sample_uint64()
        assert np.array_equal(S.centered_binomial_from_words(w, Q), ref.centered_binomial(n, Q))
        assert after.sample_uint64() == ref.sample_uint64()          # both consumed n / 2 blocks


@pytest.mark.parametrize("n", [64, 1024])
def test_weight_values_and_limbs(O, n):
    w, _ = S.words(O, 0x5EED, 1, 3, n)
    for h in (1, 32, n - 1, n):
        out = S.ternary_sparse(w, h, Q)
        assert out.shape == (3, n)
        for i, q in enumerate(Q):
            assert set(np.unique(out[i]).tolist()) <= {0, 1, q - 1}
            assert int(np.count_nonzero(out[i])) == h
            assert np.array_equal(out[i] == 1, out[0] == 1) and np.array_equal(out[i] == q - 1, out[0] == Q[0] - 1)
    # the support grows with h: the h smallest keys contain the h - 1 smallest
    small, large = S.ternary_sparse(w, 32, Q)[0] != 0, S.ternary_sparse(w, 33, Q)[0] != 0
    assert np.all(large[small]) and int(large.sum()) == 33


def test_keys_are_distinct_and_carry_the_index(O):
    w, _ = S.words(O, 9, 9, 0, 1024)
    w[5] = w[6] = w[7]                                               # equal random bits: the index still orders them
    support, _ = S.support_and_signs(w, 1024)
    assert sorted(support.tolist()) == list(range(1024))
    assert support.tolist().index(5) < support.tolist().index(6) < support.tolist().index(7)


def test_two_counters_give_different_supports(O):
    a = S.ternary_sparse(S.words(O, 77, 0, 0, 1024)[0], 32, Q)
    b = S.ternary_sparse(S.words(O, 77, 0, 512, 1024)[0], 32, Q)     # the next polynomial of the same generator
    assert not np.array_equal(a[0] != 0, b[0] != 0)


def test_every_position_and_both_signs_occur(O):
    """256 fixed seeds at N = 64, h = 16: every position is hit, with both signs (deterministic: the seeds are constants)"""
    n, h = 64, 16
    plus, minus = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    for seed in range(1, 257):
        out = S.ternary_sparse(S.words(O, seed, 0, 0, n)[0], h, Q[:1])[0]
        plus += out == 1
        minus += out == Q[0] - 1
    assert int((plus + minus).sum()) == 256 * h
    assert plus.min() > 0 and minus.min() > 0, (plus.tolist(), minus.tolist())


def test_the_choice_of_degree_and_double_angles(O):
    """K = ceil(1 + 6.5 sqrt(33 / 12)) = 12 on the chain of tests/test_gpu_bootstrap_api.py.  The float64 specification of the whole chain
    (tests/bootstrap_spec.py pipeline, the message and the integers I of tests/test_bootstrap_spec.py with |I| <= K - 1) returns m within 6.5e-06 for
    (K, degree, double angles) = (64, 79, 3).  Among ALL pairs (degree 1 .. 127, double angles 0 .. 5) that stay under 6.5e-06 with K = 12,
    the smallest is taken: fewest levels chebyshev_depth(degree) + double angles first, then the lowest degree.  That is (39, 2), depth 8."""
    n, delta, k = 1024, float(1 << 50), math.ceil(1.0 + 6.5 * math.sqrt((EPHEMERAL_WEIGHT + 1) / 12.0))
    assert k == 12
    primes = O.coeff_modulus_create(n, [60] + [50] * 17 + [60])[:-1]
    tables = E.numpy_tables(10)
    rng = np.random.default_rng(11)
    m = rng.uniform(-1.0, 1.0, n)
    integers = rng.integers(-(k - 1), k, n).astype(np.float64)
    integers[:4] = [k - 1, -(k - 1), 0, k - 1]
    t = delta * m + float(primes[0]) * integers
    chosen_depth = C.total_depth(ENCAPSULATED_DEGREE) + ENCAPSULATED_DOUBLE_ANGLES
    assert chosen_depth == 8
    under = []
    for degree in range(1, 128):
        for r in range(0, 6):
            depth = C.total_depth(degree) + r
            if depth > chosen_depth:
                continue
            got, _ = B.pipeline(t, primes, delta, k, degree, r, [3, 3, 3], [3, 3, 3], float(1 << 50), tables)
            if float(np.max(np.abs(got - m))) < 6.5e-06:
                under.append((depth, degree, r))
    best = min(under)
    got, consts = B.pipeline(t, primes, delta, k, ENCAPSULATED_DEGREE, ENCAPSULATED_DOUBLE_ANGLES, [3, 3, 3], [3, 3, 3], float(1 << 50), tables)
    print("pairs under 6.5e-06 at depth <= 8: %s; chosen %s, spec error %.3e, levels %d" % (sorted(under)[:4], best, float(np.max(np.abs(got - m))), consts["levels"]))
    assert best == (chosen_depth, ENCAPSULATED_DEGREE, ENCAPSULATED_DOUBLE_ANGLES)
    assert consts["levels"] == 3 + 8 + 3
