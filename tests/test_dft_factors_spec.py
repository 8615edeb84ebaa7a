"""tests/dft_factors_spec.py, the factored special DFT for the generator-3 slot order, against the encoder's specification (ckks_encode_spec.py)
on numpy's tables: N = 16, 64, 1024.  The bound of every comparison is the transform term of ckks_encode_spec.round_trip_bound,
8 log2(N) 2^-52 SUM |t|.  No GPU needed."""
import numpy as np
import pytest

import ckks_encode_spec as E
import dft_factors_spec as S

SIZES = [4, 6, 10]
_CACHE = {}


def _case(log_n):
    """tables, coefficients t, BR w and the encoder's slots, computed once per size and never modified"""
    if log_n not in _CACHE:
        N = 1 << log_n
        n = N // 2
        tables = E.numpy_tables(log_n)
        t = np.random.default_rng(log_n).uniform(-1, 1, N)
        z = E.simd_from_coefficients(t, tables)
        x = S.bit_reverse(t[:n], n), S.bit_reverse(t[n:], n)
        bound = 8.0 * log_n * 2.0 ** -52 * float(np.sum(np.abs(t)))
        for a in (t, *z, *x):
            a.setflags(write=False)
        _CACHE[log_n] = tables, t, x, z, bound
    return _CACHE[log_n]


def _groupings(m):
    return [[1] * m, S.default_groups(m, 3), [m]]


def _forward(tables, n, groups, x, tabs=None):
    yr, yi = x
    first = 0
    for c in groups:
        yr, yi = S.apply(S.table(tables, first, c), n, first, c, yr, yi)
        first += c
    return yr, yi


def _inverse(tables, n, groups, y):
    yr, yi = y
    first = sum(groups)
    for c in reversed(groups):
        first -= c
        yr, yi = S.apply(S.table(tables, first, c, inverse=True), n, first, c, yr, yi)
    return yr, yi


def _err(a, b):
    return max(float(np.max(np.abs(a[0] - b[0]))), float(np.max(np.abs(a[1] - b[1]))))


@pytest.mark.parametrize("log_n", SIZES)
def test_forward_groups_give_the_encoders_slots(log_n):
    """L_{m-1} ... L_0 BR w with the odd slots conjugated back is simd_from_coefficients(t), in every grouping; the groupings agree with each other"""
    tables, t, x, z, bound = _case(log_n)
    n, m = 1 << (log_n - 1), log_n - 1
    odd = (np.arange(n) & 1) == 1
    results = []
    for groups in _groupings(m):
        yr, yi = _forward(tables, n, groups, x)
        results.append((yr, yi))
        err = _err((yr, np.where(odd, -yi, yi)), z)
        print("N = %d groups %s: error %.3e (bound %.3e)" % (1 << log_n, groups, err, bound))
        assert err <= bound
    for other in results[1:]:
        assert _err(other, results[0]) <= bound


@pytest.mark.parametrize("log_n", SIZES)
def test_inverse_after_forward_is_the_identity(log_n):
    tables, t, x, z, bound = _case(log_n)
    n, m = 1 << (log_n - 1), log_n - 1
    for groups in _groupings(m):
        back = _inverse(tables, n, groups, _forward(tables, n, groups, x))
        assert _err(back, x) <= bound


@pytest.mark.parametrize("log_n", SIZES)
def test_masked_decomposition(log_n):
    """point 6: CoeffToSlot G zh = (G E) z + (G O) conj(z) with the columns of the first-applied group masked; SlotToCoeff
    z = (E G') y + (O conj(G')) conj(y) with the rows of the last-applied group masked"""
    tables, t, x, z, bound = _case(log_n)
    n, m = 1 << (log_n - 1), log_n - 1
    c = min(3, m)
    first = m - c
    odd = (np.arange(n) & 1) == 1
    zh = z[0], np.where(odd, -z[1], z[1])
    # CoeffToSlot: the top group inverse, applied to zh, against the two masked halves applied to z and conj(z)
    want = S.apply(S.table(tables, first, c, inverse=True), n, first, c, *zh)
    even_part = S.apply(S.table(tables, first, c, inverse=True, col_mask=S.MASK_EVEN), n, first, c, z[0], z[1])
    odd_part = S.apply(S.table(tables, first, c, inverse=True, col_mask=S.MASK_ODD), n, first, c, z[0], -z[1])
    assert _err((even_part[0] + odd_part[0], even_part[1] + odd_part[1]), want) <= bound
    # SlotToCoeff: y = the state before the top group; z from the row-masked halves
    lower = [1] * first
    y = _forward(tables, n, lower, x) if lower else x
    even_part = S.apply(S.table(tables, first, c, row_mask=S.MASK_EVEN), n, first, c, y[0], y[1])
    odd_part = S.apply(S.table(tables, first, c, row_mask=S.MASK_ODD, conjugate=True), n, first, c, y[0], -y[1])
    assert _err((even_part[0] + odd_part[0], even_part[1] + odd_part[1]), z) <= bound
    # a mask only removes entries, and the two masks partition the table
    full = S.table(tables, first, c)
    a, b = S.table(tables, first, c, row_mask=S.MASK_EVEN), S.table(tables, first, c, row_mask=S.MASK_ODD)
    assert np.array_equal(a + b, full) and not np.any((a != 0) & (b != 0))
    a, b = S.table(tables, first, c, col_mask=S.MASK_EVEN), S.table(tables, first, c, col_mask=S.MASK_ODD)
    assert np.array_equal(a + b, full) and not np.any((a != 0) & (b != 0))


@pytest.mark.parametrize("log_n", SIZES)
def test_diagonal_counts(log_n):
    """point 4: a product of r layers has 2^(r+1) - 1 diagonals, the multiples of the smallest lh, and 2^r where the top layer is in it; every
    listed diagonal holds a non-zero and every row holds 2^r of them"""
    tables = _case(log_n)[0]
    n, m = 1 << (log_n - 1), log_n - 1
    for first, count in [(0, 1), (0, min(3, m)), (m - 1, 1), (max(m - 3, 0), min(3, m)), (0, m)] + ([(1, 2)] if m >= 4 else []):
        ds = S.diagonal_indices(n, first, count)
        top = first + count == m
        assert len(ds) == ((1 << count) if top else (2 << count) - 1) == S.diagonal_count(n, first, count)
        assert ds == sorted(set(ds)) and all(d % (1 << first) == 0 and 0 <= d < n for d in ds)
        for inverse in (False, True):
            tab = S.table(tables, first, count, inverse=inverse)
            nonzero = (tab[..., 0] != 0) | (tab[..., 1] != 0)
            assert nonzero.any(axis=1).all()
            assert (nonzero.sum(axis=0) == (1 << count)).all()


def test_three_groups_of_three_at_1024():
    """the issue's measurement: N = 1024 in three groups of three layers has 15, 15 and 8 diagonals"""
    assert [S.diagonal_count(512, f, 3) for f in (0, 3, 6)] == [15, 15, 8]
    assert S.default_groups(9, 3) == [3, 3, 3] and S.default_groups(9) == [3, 3, 3] and S.default_groups(13) == [4, 3, 3, 3] and S.default_groups(3) == [3]


def test_table_is_entry_by_entry():
    """the vectorised table is entry() for every (diagonal, row), options included: the same words"""
    tables = _case(6)[0]
    n = 32
    for first, count, inverse, cm, rm, conj, const in [(1, 2, True, 0, 0, False, 0.7), (0, 3, False, 2, 0, True, -1.25), (3, 2, False, 0, 1, False, 1.0), (2, 3, True, 1, 0, False, 3.0)]:
        tab = S.table(tables, first, count, inverse=inverse, col_mask=cm, row_mask=rm, conjugate=conj, constant=const)
        for a, d in enumerate(S.diagonal_indices(n, first, count)):
            for i in range(n):
                col = (i + d) % n
                e = S.entry(tables, first, count, inverse, i, col, const)
                keep = (rm == 0 or (i & 1) == (rm == 2)) and (cm == 0 or (col & 1) == (cm == 2))
                if e is None or not keep:
                    want = (0.0, 0.0)
                else:
                    want = (e[0], -e[1] if conj else e[1])
                assert (tab[a, i, 0], tab[a, i, 1]) == want, (first, count, a, i)


def test_a_constant_scales_the_map():
    tables, t, x, z, bound = _case(6)
    n = 32
    plain = S.apply(S.table(tables, 1, 3), n, 1, 3, *x)
    scaled = S.apply(S.table(tables, 1, 3, constant=0.375), n, 1, 3, *x)
    assert _err((plain[0] * 0.375, plain[1] * 0.375), scaled) <= bound
