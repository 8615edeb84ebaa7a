"""tests/bootstrap_spec.py against independent statements (CPU): the mu vector against the oracle's forward transform of X^(N/2) and against a direct
evaluation at the roots, the slots of X^(N/2) by tests/ckks_encode_spec.py, split / join identities, and the float64 pipeline t = D m + q0 I -> m."""
import math

import numpy as np
import pytest

import bootstrap_spec as B
import ckks_encode_spec as E

K, DEGREE, DOUBLE_ANGLES = 64, 79, 3      # the choice of tests/test_gpu_bootstrap_api.py: depth 7 + 3


@pytest.mark.parametrize("n", [16, 64, 1024])
@pytest.mark.parametrize("bits", [40, 50, 60])
def test_mu_is_the_forward_transform_of_the_monomial(O, n, bits):
    q = O.coeff_modulus_create(n, [bits, 60])[0]
    log_n = n.bit_length() - 1
    tables = O.NTTTables(log_n, q)
    iota = B.iota_of(n, q, tables.root)
    assert tables.root_power(1) == iota                      # the table entry the kernels read
    mu = B.mu_vector(n, q, iota)
    mono = np.zeros(n, dtype=np.uint64)
    mono[n // 2] = 1
    assert [int(v) for v in O.ntt_forward(mono, 1, 1, log_n, [tables])] == mu
    assert B.monomial_transform_direct(n, q, tables.root) == mu
    # split / join on integer rows: join(split) = 2a, and mu squared is -1
    rng = np.random.default_rng(n + bits)
    a, b = ([int(v) for v in rng.integers(0, q, n, dtype=np.uint64)] for _ in range(2))
    a[0], b[0], a[n - 1], b[n - 1] = 0, q - 1, q - 1, 0
    s, d = B.split_rows(a, b, mu, q)
    assert B.join_rows(s, d, mu, q) == [2 * v % q for v in a]
    assert all(m * m % q == q - 1 for m in mu)


@pytest.mark.parametrize("log_n", [4, 6, 10])
def test_the_slots_of_the_monomial_are_i_with_alternating_sign(log_n):
    n = 1 << log_n
    t = np.zeros(n)
    t[n // 2] = 1.0
    re, im = E.simd_from_coefficients(t, E.numpy_tables(log_n))
    want = 1j * np.where(np.arange(n // 2) % 2 == 0, 1.0, -1.0)
    assert np.max(np.abs(np.asarray(re) + 1j * np.asarray(im) - want)) < 1e-12


def test_the_pipeline_returns_the_message(O):
    """bound, from its parts: the sine's cubic term 6.58 (D / q0)^2 |m|, plus the interpolant's sup-norm error on a fine grid times 2^double_angles
    times q0 / D; a margin of 4 for float64 accumulation.  The choice (K, degree, double_angles) = (64, 79, 3) must put it below 1e-6 q0 / D.
    The chain is the one of tests/test_gpu_bootstrap_api.py: N = 1024, a 60-bit q0, seventeen 50-bit primes, groups 3 + 3 + 3 twice, weights at 2^50."""
    n, delta = 1024, float(1 << 50)
    primes = O.coeff_modulus_create(n, [60] + [50] * 17 + [60])[:-1]
    q0 = float(primes[0])
    tables = E.numpy_tables(10)
    rng = np.random.default_rng(11)
    m = rng.uniform(-1.0, 1.0, n)
    integers = rng.integers(-(K - 1), K, n).astype(np.float64)
    integers[:4] = [K - 1, -(K - 1), 0, K - 1]
    got, k = B.pipeline(delta * m + q0 * integers, primes, delta, K, DEGREE, DOUBLE_ANGLES, [3, 3, 3], [3, 3, 3], float(1 << 50), tables)
    assert k["levels"] == 3 + 10 + 3
    assert abs(k["part"] * K / float(primes[len(primes) - 3 - 1]) - 1.0) < 1e-12      # EvalMod's working scale is the prime it first divides by
    assert abs(k["c2"] * k["s2"] / q0 - 1.0) < 1e-12
    e = B.interpolant_error(K, DEGREE, DOUBLE_ANGLES)
    bound = 4.0 * (6.58 * (delta / q0) ** 2 * 1.0 + e * 2 ** DOUBLE_ANGLES * (q0 / delta))
    err = float(np.max(np.abs(got - m)))
    print("pipeline error %.3e, bound %.3e (interpolant %.3e), limit %.3e" % (err, bound, e, 1e-6 * q0 / delta))
    assert bound < 1e-6 * q0 / delta
    assert err <= bound
    assert math.isclose(float(B.eval_mod(0.0, K, DEGREE, DOUBLE_ANGLES)), 0.0, abs_tol=1e-9)
    # the schedule of chebyshev_spec and numpy's chebval state the same function
    x = rng.integers(-(K - 1), K, 64) + rng.uniform(-2.0 ** -10, 2.0 ** -10, 64)
    c = B.interpolant(K, DEGREE, DOUBLE_ANGLES)
    assert np.max(np.abs(B.eval_mod_scheduled(x, K, c, DOUBLE_ANGLES) - B.eval_mod(x, K, DEGREE, DOUBLE_ANGLES, c))) < 1e-9
