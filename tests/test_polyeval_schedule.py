"""The schedule of Evaluator::evaluate_polynomial (tests/polyeval_spec.py restates troy/troy.h): k, g, the power set and the depth formula
for d = 1..40, and a noise-free simulation on exact rationals: every addend of the final sum has the same scale and value / scale = p(x)
(no GPU needed)."""
import os
from fractions import Fraction

import numpy as np
import pytest

import polyeval_spec as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("d", range(1, 41))
def test_schedule(d):
    k, g, needed, depth = S.schedule(d)
    if d <= 1:
        assert (k, g, needed, depth) == (1, 1, set(), 1)
        return
    assert k & (k - 1) == 0 and k * k >= d + 1 and (k // 2) ** 2 < d + 1          # the smallest power of two with k^2 >= d + 1
    assert (g - 1) * k < d + 1 <= g * k and g >= 2
    assert needed == set(range(2, k)) | {k} | {j * k for j in range(1, g)}
    assert depth == max(S.clog2((g - 1) * k), S.clog2(k) + 1) + 1
    for m in needed:                                                              # every factor of a needed power is needed or x itself
        a, b = S.split(m)
        assert a + b == m and a & (a - 1) == 0 and (a == b or a > b)
        assert max(S.power_depth(a), S.power_depth(b)) + 1 == S.power_depth(m)
    # the babies leave room for the leaf's own division above the recombination level, the giants reach it
    assert S.power_depth(k - 1) + 1 <= depth - 1 and S.power_depth((g - 1) * k) <= depth - 1


def test_known_points():
    assert S.schedule(2)[:2] == (2, 2) and S.schedule(2)[3] == 3
    assert S.schedule(7)[:2] == (4, 2) and S.schedule(7)[3] == 4
    assert S.schedule(12)[:2] == (4, 4) and S.schedule(12)[3] == 5
    assert S.schedule(63)[:2] == (8, 8) and S.schedule(63)[3] == 7


def test_header_states_the_schedule():
    text = open(os.path.join(ROOT, "troy-nova_amd", "troy", "troy.h")).read()
    start = text.index("ADDITION to the reference's interface: real linear combinations of ciphertexts and polynomial evaluation")
    block = " ".join(text[start:text.index("void linear_combinations(")].replace("//", " ").split())      # the comment's line breaks do not matter
    for word in ("k = the smallest power of two with k^2 >= d + 1", "g = ceil((d + 1) / k)", "depth(x^m) = ceil(log2 m)",
                 "max(ceil(log2((g-1)k)), log2 k + 1) + 1", "Chebyshev", "rounded half away from zero", "2^62"):
        assert word in block, word


@pytest.fixture(scope="module")
def primes(pkg):
    q = pkg.capi.coeff_modulus_create(8192, [60] + [40] * 6 + [60])
    return [int(x) for x in q[:-1]]      # the data primes; the special prime takes no part


@pytest.mark.parametrize("d", [1, 2, 3, 7, 12, 15, 16, 31, 40])
def test_simulation_scales_match_and_value_is_p(primes, d):
    rng = np.random.default_rng(d)
    coefficients = [Fraction(float(c)) for c in rng.uniform(-1, 1, d + 1)]
    k, g, needed, depth = S.schedule(d)
    if depth + 1 > len(primes):
        with pytest.raises(AssertionError):
            S.simulate(Fraction(1, 3), coefficients, 1 << 40, primes)
        return
    for message in (Fraction(-1), Fraction(7, 10), Fraction(-1, 3), Fraction(1)):
        addends, out, muls = S.simulate(message, coefficients, 1 << 40, primes)
        assert len({a.scale for a in addends}) == 1 and all(a.limbs == out.limbs for a in addends)
        assert out.scale == 1 << 40 and out.limbs == len(primes) - depth
        assert sorted(muls) == sorted(needed)                       # one multiplication per needed power, none else
        want = sum(c * message ** m for m, c in enumerate(coefficients))
        # noise-free: only the roundings of the encodings and divisions remain, each below one unit of a 2^40 scale times the operands
        assert abs(Fraction(out.value) / out.scale - want) < Fraction(d + 8, 1 << 36)
