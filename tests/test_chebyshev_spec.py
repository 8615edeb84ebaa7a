"""tests/chebyshev_spec.py against itself and against numpy (no GPU): the product-plus-affine step in two forms that must agree, the
leaf-coefficient solve and the ladder against numpy.polynomial.chebyshev.chebval, the depth formula."""
import numpy as np
import pytest
from numpy.polynomial import chebyshev as npcheb

import chebyshev_spec as S
from polyeval_spec import clog2, schedule

Q60 = [(1 << 60) - 93, (1 << 60) - 107, (1 << 60) - 173]      # the contract is plain modular arithmetic: any odd 60- and 40-bit moduli do
Q40 = [(1 << 40) - 87, (1 << 40) - 167, (1 << 40) - 195]


def _case(rng, q, n, c_limbs, top=False):
    L = len(q)
    word = (lambda l, size: np.full(size, q[l] - 1, dtype=np.uint64)) if top else (lambda l, size: rng.integers(0, q[l], size=size, dtype=np.uint64))
    a = np.stack([np.stack([word(l, n) for l in range(L)]) for _ in range(2)])
    b = np.stack([np.stack([word(l, n) for l in range(L)]) for _ in range(2)])
    c = None
    if c_limbs:
        c = np.full((2, c_limbs, n), np.uint64((1 << 64) - 1), dtype=np.uint64)      # limbs beyond L hold words no modulus admits
        for l in range(L):
            c[:, l] = np.stack([word(l, n), word(l, n)])
    return a, b, c


@pytest.mark.parametrize("q", [Q60, Q40, Q60[:2]])
@pytest.mark.parametrize("extra", [None, 0, 2])      # no addend, an addend with L limbs, a taller one
def test_step_direct_equals_fold(q, extra):
    rng = np.random.default_rng(len(q) * 7 + (extra or 0))
    L = len(q)
    for alpha_of, w_of in [(lambda l: 1, lambda l: 0), (lambda l: 2, lambda l: 1), (lambda l: q[l] - 1, lambda l: q[l] - 1),
                           (lambda l: int(rng.integers(0, q[l])), lambda l: int(rng.integers(0, q[l])))]:
        a, b, c = _case(rng, q, 16, 0 if extra is None else L + extra)
        alpha, w = [alpha_of(l) for l in range(L)], [w_of(l) for l in range(L)]
        for k in (None, [q[l] - 1 for l in range(L)], [int(rng.integers(0, q[l])) for l in range(L)]):
            direct, fold = S.step_direct(q, a, b, c, alpha, w, k), S.step_fold(q, a, b, c, alpha, w, k)
            assert direct.dtype == np.uint64 and np.array_equal(direct, fold)
            assert all((direct[:, l] < np.uint64(q[l])).all() for l in range(L))


def test_step_with_every_word_at_the_top():
    """every input word and every scalar q - 1 under 60-bit moduli: q - 1 = -1, so every word of P has a closed form"""
    q, L = Q60, len(Q60)
    a, b, c = _case(np.random.default_rng(0), q, 8, L, top=True)
    top = [v - 1 for v in q]
    direct = S.step_direct(q, a, b, c, top, top, top)
    assert np.array_equal(direct, S.step_fold(q, a, b, c, top, top, top))
    for l in range(L):
        # alpha * 1 + w * (q - 1) + k = -1 + 1 - 1 = -1;  alpha * 2 + 1 = -1;  alpha * 1 = -1
        assert (direct[0, l] == np.uint64(q[l] - 1)).all() and (direct[1, l] == np.uint64(q[l] - 1)).all() and (direct[2, l] == np.uint64(q[l] - 1)).all()


def test_step_is_the_chebyshev_recurrence_on_small_integers():
    """a = (T_a, 0), b = (T_b, 0), c = (T_c, 0) as constants: P_0 = 2 T_a T_b - T_c, P_1 = P_2 = 0"""
    q = Q40[:2]
    ta, tb, tc = 7, 97, 26                      # T_2(2), T_4(2) ... any integers do
    mk = lambda v: np.stack([np.full((2, 4), v, dtype=np.uint64), np.zeros((2, 4), dtype=np.uint64)])
    p = S.step_direct(q, mk(ta), mk(tb), mk(tc), [2, 2], [v - 1 for v in q], None)
    assert (p[0] == np.uint64(2 * ta * tb - tc)).all() and not p[1:].any()


@pytest.mark.parametrize("d", [1, 2, 7, 12, 31, 127])
def test_schedule_evaluates_the_chebyshev_series(d):
    rng = np.random.default_rng(d)
    coeffs = rng.uniform(-1, 1, d + 1)
    coeffs[d] = 0.5 + abs(coeffs[d]) / 2      # the stated degree is the real one
    y = np.concatenate([rng.uniform(-1, 1, 200), [-1.0, 1.0, 0.0]])
    got = S.evaluate(y, list(coeffs))
    want = npcheb.chebval(y, coeffs)
    # float64: each T_m carries a few ulp of a value <= 1 per recurrence step (depth <= 7), the sum has d + 1 terms of magnitude <= 2
    assert np.max(np.abs(got - want)) <= 64 * (d + 1) * np.finfo(np.float64).eps
    # trailing zeros do not change the degree
    assert np.array_equal(S.evaluate(y, list(coeffs) + [0.0, 0.0]), got)


@pytest.mark.parametrize("d", [2, 7, 12, 31, 127])
def test_ladder_values_and_batches(d):
    y = np.linspace(-1, 1, 41)
    t, batches = S.ladder(y, d)
    for m, v in t.items():
        assert np.max(np.abs(v - np.cos(m * np.arccos(y)))) <= 1e-12, m
    k, g, _, _ = schedule(d)
    assert set(range(2, k)) <= set(t) and all(j * k in t for j in range(1, g))
    for dep, ms in batches.items():      # one batched call per depth, every member exactly at that depth
        assert all(S.depth_of(m) == dep == clog2(m) for m in ms)
    assert sorted(m for ms in batches.values() for m in ms) == sorted(S.needed(d))


@pytest.mark.parametrize("d", list(range(1, 128)))
def test_depth_formula(d):
    k, g, _, depth = schedule(d)
    assert S.total_depth(d) == depth
    if d <= 1:
        assert depth == 1 and not S.needed(d)
        return
    assert k * k >= d + 1 and (k // 2) ** 2 < d + 1 and g == -(-(d + 1) // k)
    rec = max(clog2((g - 1) * k), clog2(k) + 1)
    assert depth == rec + 1
    # every T_m the schedule needs is ready by the recombination level; the leaves (one rescale below the deepest baby) too
    assert max(S.depth_of(m) for m in S.needed(d)) <= rec and clog2(k) + 1 <= rec
    assert depth <= 8      # d <= 127


def test_degree_cap_and_zero_vector():
    with pytest.raises(ValueError):
        S.evaluate(np.zeros(3), [0.0] * 5)
    with pytest.raises(ValueError):
        S.evaluate(np.zeros(3), [0.0] * 128 + [1.0])
    S.evaluate(np.zeros(3), [0.0] * 127 + [1.0])
