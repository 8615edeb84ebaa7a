"""The specification of the BFV inner product (tests/bfv_dot_spec.py) against the oracle's own multiply (no GPU)."""
import numpy as np
import pytest

from bfv_dot_spec import BfvDotSpec

CHAINS = [(1024, [40, 40, 40], 65537), (2048, [50, 50, 50, 50], 786433), (1024, [60, 40, 40, 60], 65537)]


@pytest.mark.parametrize("n,bits,t", CHAINS)
def test_one_term_is_the_reference_multiply(O, n, bits, t):
    q = O.coeff_modulus_create(n, bits)
    L = len(q) - 1
    ctx = O.Context("bfv", n, q, t)
    spec = BfvDotSpec(O, n, q, L, t)
    a, b = ctx.random_ct(3, 2, L), ctx.random_ct(5, 2, L)
    assert np.array_equal(spec.dot([a], [b]), ctx.bfv_multiply(L, a, b))
    assert np.array_equal(spec.dot([a], [a]), ctx.bfv_multiply(L, a, a))


@pytest.mark.parametrize("terms", [2, 7])
def test_repeated_pair_is_the_scaled_tensor_product(O, terms):
    n, t = 1024, 65537
    q = O.coeff_modulus_create(n, [40, 40, 40])
    ctx = O.Context("bfv", n, q, t)
    spec = BfvDotSpec(O, n, q, 2, t)
    a, b = ctx.random_ct(11, 2, 2), ctx.random_ct(13, 2, 2)
    assert np.array_equal(spec.repeated(a, b, terms), spec.dot([a] * terms, [b] * terms))
