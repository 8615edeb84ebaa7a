"""The algebra of the fused BGV chain on a tiny ring (N = 8, three 20-bit primes, t = 17 and t = 2): the derivation with ONE forward transform
per output limb equals multiply -> relinearize -> mod-switch composed, in exact integers (tests/bgv_chain_spec.py)."""
import pytest

import bgv_chain_spec as S

Q = S.ntt_primes(3)
L = 2      # two data limbs and the special prime: the only level of a three-prime chain with a next level


def test_transform_is_a_negacyclic_ntt():
    q = Q[0]
    a, b = [3, 1, 4, 1, 5, 9, 2, 6], [2, 7, 1, 8, 2, 8, 1, 8]
    want = [0] * S.N
    for i, x in enumerate(a):
        for j, y in enumerate(b):
            k = i + j
            want[k % S.N] = (want[k % S.N] + (x * y if k < S.N else -x * y)) % q
    assert S.intt(S.mul(S.ntt(a, q), S.ntt(b, q), q), q) == want
    assert all(p.bit_length() == 20 and p % (2 * S.N) == 1 for p in Q) and len(set(Q)) == 3


@pytest.mark.parametrize("t", [17, 2])
@pytest.mark.parametrize("seed", range(6))
def test_fused_equals_composed_on_random_inputs(t, seed):
    a, b, keys = S.random_case(seed, Q, L)
    got = S.fused(a, b, keys, Q, L, t)
    assert got == S.composed(a, b, keys, Q, L, t)
    assert all(0 <= v < Q[j] for comp in got for j, row in enumerate(comp) for v in row)


@pytest.mark.parametrize("t", [17, 2])
def test_fused_equals_composed_on_edge_rows(t):
    _, _, keys = S.random_case(99, Q, L)
    top = S.constant_ct(Q, L, lambda q: q - 1)
    zero = S.constant_ct(Q, L, lambda q: 0)
    rnd, _, _ = S.random_case(5, Q, L)
    assert S.fused(top, top, keys, Q, L, t) == S.composed(top, top, keys, Q, L, t)
    assert S.fused(rnd, zero, keys, Q, L, t) == S.composed(rnd, zero, keys, Q, L, t)
    # a zero operand: the division of zero is zero
    assert S.fused(rnd, zero, keys, Q, L, t) == [[[0] * S.N for _ in range(L - 1)] for _ in range(2)]
    assert S.fused(zero, zero, keys, Q, L, t) == S.composed(zero, zero, keys, Q, L, t)


def test_t_two_takes_the_unit_inverses():
    """t = 2: both q^-1 mod t are 1, the branch the kernels special-case"""
    assert pow(Q[-1], -1, 2) == 1 and pow(Q[L - 1], -1, 2) == 1


@pytest.mark.parametrize("t", [17, 2])
def test_dropping_the_key_switch_correction_is_caught(t):
    """the mutation of the GPU tests' check, on the specification: without dk_j(s) qk^-1 the words differ"""
    a, b, keys = S.random_case(1, Q, L)
    assert S.fused(a, b, keys, Q, L, t, drop_key_correction=True) != S.composed(a, b, keys, Q, L, t)
