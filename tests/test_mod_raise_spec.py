"""The two restatements of the ModRaise contract (tests/mod_raise_spec.py) agree: big integers against mixed-radix digits with a lexicographic
centring and a Horner per target prime -- on random words, on the planted boundary values and on values whose top digits tie with floor(Q/2)."""
import numpy as np
import pytest

import mod_raise_spec as S

CHAINS = [(32, [30] * 18), (4096, [60, 40, 40, 40, 40, 60]), (8192, [50] * 6)]
CASES = [(0, 1, 4), (0, 16, 17), (0, 5, 18), (1, 1, 6), (1, 2, 6), (1, 3, 6), (1, 5, 6), (2, 2, 6), (2, 1, 2)]


def _primes(O, chain):
    n, bits = CHAINS[chain]
    return [int(v) for v in O.coeff_modulus_create(n, bits)]


def _check(primes, L_in, L_out, values):
    """both forms on the residues of `values`; the properties of the contract"""
    inp = primes[:L_in]
    Q = S.product(inp)
    res = S.residues_of(values, inp)
    want = S.mod_raise_rows(res, primes, L_in, L_out)
    got = S.mod_raise_mixed_radix(res, primes, L_in, L_out)
    assert want.shape == (L_out, len(values)) and np.array_equal(got, want)
    assert np.array_equal(want[:L_in], res)                                   # the low rows are the input
    for k, v in enumerate(values):
        x = S.centre(int(v) % Q, Q)
        assert -Q < 2 * x <= Q                                                # |x| <= Q/2, +Q/2 included, -Q/2 excluded
        for j in range(L_out):
            assert int(want[j, k]) == x % primes[j] and int(want[j, k]) < primes[j]
    return want


@pytest.mark.parametrize("chain,L_in,L_out", CASES)
def test_forms_agree_on_random_words(O, chain, L_in, L_out):
    primes = _primes(O, chain)
    rng = np.random.default_rng(1000 * chain + 10 * L_in + L_out)
    Q = S.product(primes[:L_in])
    values = [int.from_bytes(rng.bytes(8 * L_in + 8), "little") % Q for _ in range(48)]
    _check(primes, L_in, L_out, values)
    xs = [S.centre(v, Q) for v in values]
    assert min(xs) < 0 < max(xs)


@pytest.mark.parametrize("chain,L_in,L_out", CASES)
def test_forms_agree_on_planted_values(O, chain, L_in, L_out):
    primes = _primes(O, chain)
    inp = primes[:L_in]
    Q, q0 = S.product(inp), inp[0]
    values = S.planted_values(inp)
    want = _check(primes, L_in, L_out, values)
    # what the planted values are, modulo a new prime: 0, 1, -1, the two sides of the half
    j = L_in
    qj = primes[j]
    h = Q // 2
    assert [int(w) for w in want[j][:6]] == [0, 1, qj - 1, h % qj, (h + 1 - Q) % qj, qj - 1]
    if L_in > 1:                                                              # (with one prime floor(Q/2) +- q_0 is floor(Q/2) again)
        assert [int(w) for w in want[j][6:]] == [(h + q0 - Q) % qj, (h - q0) % qj]


@pytest.mark.parametrize("chain,L_in,L_out", CASES)
def test_forms_agree_where_the_top_digits_tie(O, chain, L_in, L_out):
    primes = _primes(O, chain)
    inp = primes[:L_in]
    rng = np.random.default_rng(7 + L_in)
    values = S.tie_values(inp, rng)
    _check(primes, L_in, L_out, values)
    half = S.digits_of_integer(S.product(inp) // 2, inp)
    # the set holds, for every digit position k, a value that ties above k and differs at k
    for k in range(L_in):
        assert any(S.digits_of_integer(v, inp)[k + 1:] == half[k + 1:] and S.digits_of_integer(v, inp)[k] != half[k] for v in values), k
    # and floor(Q/2) itself, where no digit differs: not above the half
    assert S.product(inp) // 2 in values
    assert not S.above_half(half, half)


def test_digits_are_the_positional_form(O):
    primes = _primes(O, 1)
    rng = np.random.default_rng(3)
    Q = S.product(primes)
    for _ in range(32):
        X = int.from_bytes(rng.bytes(40), "little") % Q
        col = [X % q for q in primes]
        d = S.mixed_radix_digits(col, primes)
        assert d == S.digits_of_integer(X, primes) and S.integer_of_digits(d, primes) == X
        assert S.compose(np.array(col, dtype=object).reshape(-1, 1), primes) == [X]
