"""tests/scalar_sums_spec.py is the contract of troyn_scalar_weighted_sums: it agrees with the term-by-term fold, states the constant rule
in both modes and never reads a limb at or beyond nmod of a taller input (no GPU needed)."""
import numpy as np
import pytest

import scalar_sums_spec as S

MODULI = [(1 << 40) - 87, (1 << 59) + 21 * (1 << 6) + 1, 1099511480321]      # any moduli do: the contract is plain modular arithmetic


def _case(seed, terms, slots, batch=2, pcount=2, n=8, extra=(0, 1, 2)):
    rng = np.random.default_rng(seed)
    nmod = len(MODULI)
    inputs = []
    for t in range(terms):
        rows = nmod + extra[t % len(extra)]
        x = np.zeros((batch, pcount, rows, n), dtype=np.uint64)
        for l in range(rows):
            q = MODULI[l] if l < nmod else (1 << 64) - 1
            x[:, :, l, :] = rng.integers(0, q, size=(batch, pcount, n), dtype=np.uint64)
        inputs.append(x)
    scalars = [[[int(rng.integers(0, q, dtype=np.uint64)) for q in MODULI] for _ in range(terms)] for _ in range(slots)]
    constants = [[int(rng.integers(0, q, dtype=np.uint64)) for q in MODULI] for _ in range(slots)]
    return inputs, scalars, constants


@pytest.mark.parametrize("terms,slots", [(1, 1), (3, 2), (9, 5)])
@pytest.mark.parametrize("mode", [None, False, True])
def test_spec_agrees_with_the_fold(terms, slots, mode):
    inputs, scalars, constants = _case(7 + terms, terms, slots)
    c = None if mode is None else constants
    a = S.scalar_weighted_sums(MODULI, inputs, scalars, c, bool(mode))
    b = S.fold_term_by_term(MODULI, inputs, scalars, c, bool(mode))
    assert a.shape == (slots, 2, 2, len(MODULI), 8) and np.array_equal(a, b)
    for l, q in enumerate(MODULI):
        assert int(a[:, :, :, l, :].max()) < q


def test_extreme_words():
    """scalars and inputs 0, 1 and q - 1"""
    n = 4
    x = np.zeros((1, 2, 3, n), dtype=np.uint64)
    for l, q in enumerate(MODULI):
        x[0, :, l, :] = [0, 1, q - 1, q - 1]
    scalars = [[[q - 1 for q in MODULI]], [[1] * 3], [[0] * 3]]
    out = S.scalar_weighted_sums(MODULI, [x], scalars)
    for l, q in enumerate(MODULI):
        assert out[0, 0, 0, l].tolist() == [0, q - 1, 1, 1]        # (q-1)(q-1) = 1
        assert out[1, 0, 1, l].tolist() == [0, 1, q - 1, q - 1]
        assert not out[2, :, :, l].any()


def test_constant_rule_in_both_modes():
    inputs, scalars, constants = _case(3, 2, 2, pcount=3)
    base = S.scalar_weighted_sums(MODULI, inputs, scalars)
    every = S.scalar_weighted_sums(MODULI, inputs, scalars, constants, False)
    first = S.scalar_weighted_sums(MODULI, inputs, scalars, constants, True)
    for s in range(2):
        for l, q in enumerate(MODULI):
            want = (base[s, :, 0, l, :].astype(object) + constants[s][l]) % q
            assert np.array_equal(every[s, :, 0, l, :].astype(object), want)
            assert np.array_equal(first[s, :, 0, l, 0].astype(object), want[:, 0])
            assert np.array_equal(first[s, :, 0, l, 1:], base[s, :, 0, l, 1:])
    assert np.array_equal(every[:, :, 1:], base[:, :, 1:]) and np.array_equal(first[:, :, 1:], base[:, :, 1:])


def test_limbs_beyond_nmod_are_not_read():
    inputs, scalars, constants = _case(5, 3, 2)
    want = S.scalar_weighted_sums(MODULI, inputs, scalars, constants, False)
    nmod = len(MODULI)
    changed = []
    for x in inputs:
        y = x.copy()
        y[:, :, nmod:, :] ^= np.uint64(0x5555555555555555)
        changed.append(y)
    assert any(x.shape[2] > nmod for x in inputs)
    assert np.array_equal(S.scalar_weighted_sums(MODULI, changed, scalars, constants, False), want)
    cut = [x[:, :, :nmod, :] for x in inputs]
    assert np.array_equal(S.scalar_weighted_sums(MODULI, cut, scalars, constants, False), want)
