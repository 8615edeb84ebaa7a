"""tests/sparse_bootstrap_spec.py against independent statements (CPU): the sub-ring factoring against the direct evaluation of p(Y) at zeta^(s 3^j),
the n = N/2 table against dft_factors_spec.table bit for bit, SubSum on exact integers, and the float64 chain t = D p(Y) + q0 I(X) -> p with dense I.
The bound of every transform comparison is the one of tests/test_dft_factors_spec.py, 8 log2(N) 2^-52 SUM |t|."""
import numpy as np
import pytest

import bootstrap_spec as B
import ckks_encode_spec as E
import dft_factors_spec as D
import sparse_bootstrap_spec as S

CASES = [(16, 2), (64, 8), (1024, 64), (1024, 256)]
K, DEGREE, DOUBLE_ANGLES = 64, 79, 3      # the choice of tests/test_gpu_bootstrap_api.py
_CACHE = {}


def _case(big_n, n):
    """the full ring's tables, the 2n coefficients of p, BR w on log2 n bits, the direct slots and the bound: computed once, never modified"""
    if (big_n, n) not in _CACHE:
        log_n = D.log2_exact(big_n)
        tables = E.numpy_tables(log_n)
        t = np.random.default_rng(big_n + n).uniform(-1, 1, 2 * n)
        z = S.direct_slots(t, big_n)
        x = D.bit_reverse(t[:n], n), D.bit_reverse(t[n:], n)
        bound = 8.0 * log_n * 2.0 ** -52 * float(np.sum(np.abs(t)))
        for a in (t, *z, *x):
            a.setflags(write=False)
        _CACHE[(big_n, n)] = tables, t, x, z, bound
    return _CACHE[(big_n, n)]


def _groupings(m):
    out = [[1] * m, D.default_groups(m, 3), [m]]
    return [g for i, g in enumerate(out) if g not in out[:i]]


def _forward(tables, n, groups, x):
    yr, yi = x
    first = 0
    for c in groups:
        yr, yi = S.apply(S.table(tables, n, first, c), n, first, c, yr, yi)
        first += c
    return yr, yi


def _inverse(tables, n, groups, y):
    yr, yi = y
    first = sum(groups)
    for c in reversed(groups):
        first -= c
        yr, yi = S.apply(S.table(tables, n, first, c, inverse=True), n, first, c, yr, yi)
    return yr, yi


def _err(a, b):
    return max(float(np.max(np.abs(a[0] - b[0]))), float(np.max(np.abs(a[1] - b[1]))))


@pytest.mark.parametrize("big_n,n", CASES)
def test_forward_groups_give_the_direct_slots(big_n, n):
    """L_{m'-1} ... L_0 BR w with the odd slots conjugated back is p at zeta^(s 3^j), in every grouping"""
    tables, t, x, z, bound = _case(big_n, n)
    m = D.log2_exact(n)
    odd = (np.arange(n) & 1) == 1
    for groups in _groupings(m):
        yr, yi = _forward(tables, n, groups, x)
        err = _err((yr, np.where(odd, -yi, yi)), z)
        print("N = %d n = %d groups %s: error %.3e (bound %.3e)" % (big_n, n, groups, err, bound))
        assert err <= bound
        assert _err(_inverse(tables, n, groups, (yr, yi)), x) <= bound


@pytest.mark.parametrize("big_n,n", CASES)
def test_the_full_ring_slots_are_the_direct_slots_tiled(big_n, n):
    """the encoder's specification on p(X^s): the N/2 slots are the n direct ones repeated s times"""
    tables, t, x, z, bound = _case(big_n, n)
    s = big_n // (2 * n)
    full = np.zeros(big_n)
    full[::s] = t
    zr, zi = E.simd_from_coefficients(full, tables)
    assert _err((zr, zi), (np.tile(z[0], s), np.tile(z[1], s))) <= bound


@pytest.mark.parametrize("big_n,n", CASES)
def test_masked_decomposition(big_n, n):
    """the even / odd masks carry over: n is even"""
    tables, t, x, z, bound = _case(big_n, n)
    m = D.log2_exact(n)
    c = min(3, m)
    first = m - c
    odd = (np.arange(n) & 1) == 1
    zh = z[0], np.where(odd, -z[1], z[1])
    want = S.apply(S.table(tables, n, first, c, inverse=True), n, first, c, *zh)
    even_part = S.apply(S.table(tables, n, first, c, inverse=True, col_mask=S.MASK_EVEN), n, first, c, z[0], z[1])
    odd_part = S.apply(S.table(tables, n, first, c, inverse=True, col_mask=S.MASK_ODD), n, first, c, z[0], -z[1])
    assert _err((even_part[0] + odd_part[0], even_part[1] + odd_part[1]), want) <= bound
    y = _forward(tables, n, [1] * first, x) if first else x
    even_part = S.apply(S.table(tables, n, first, c, row_mask=S.MASK_EVEN), n, first, c, y[0], y[1])
    odd_part = S.apply(S.table(tables, n, first, c, row_mask=S.MASK_ODD, conjugate=True), n, first, c, y[0], -y[1])
    assert _err((even_part[0] + odd_part[0], even_part[1] + odd_part[1]), z) <= bound


@pytest.mark.parametrize("log_n", [4, 6, 10])
def test_full_n_is_the_full_table_bit_for_bit(log_n):
    tables = E.numpy_tables(log_n)
    n, m = 1 << (log_n - 1), log_n - 1
    bits = lambda a: np.ascontiguousarray(a).view(np.uint64)      # noqa: E731
    for first, count in {(0, 1), (0, min(3, m)), (m - 1, 1), (max(m - 3, 0), min(3, m)), (0, m)}:
        for kw in ({}, {"inverse": True}, {"inverse": True, "col_mask": 1, "constant": 0.9}, {"row_mask": 2, "conjugate": True, "constant": -1.0 / 3.0}):
            assert np.array_equal(bits(S.table(tables, n, first, count, **kw)), bits(D.table(tables, first, count, **kw))), (first, count, kw)


def test_sparse_table_is_the_corner_of_the_full_one():
    """M_sub[i][j] = M_full[i][j] for i, j < n: every entry of the n-row table is the full ring's entry at the same (row, column), word for word"""
    tables = E.numpy_tables(10)
    n = 64
    for first, count, kw in ((1, 3, {"inverse": True, "constant": 0.7}), (3, 3, {"row_mask": 2, "conjugate": True}), (0, 6, {"inverse": True, "col_mask": 1})):
        sparse, full = S.table(tables, n, first, count, **kw), D.table(tables, first, count, **kw)
        df = D.diagonal_indices(512, first, count)
        for a, d in enumerate(S.diagonal_indices(n, first, count)):
            for i in range(n):
                diff = ((i + d) % n - i) % 512
                want = full[df.index(diff)][i] if diff in df else np.zeros(2)
                assert np.array_equal(sparse[a][i], want), (first, count, a, i)


@pytest.mark.parametrize("big_n,n", [(16, 2), (16, 4), (64, 8), (64, 2), (256, 32), (64, 32)])
def test_sub_sum_on_integers(big_n, n):
    """SUM_i sigma_{3^(n i)}(t) = s times the Y-part of t, exactly; the staged product equals the full sum for radix 2, 4 and s"""
    rng = np.random.default_rng(big_n * 7 + n)
    s = big_n // (2 * n)
    t = [int(v) << 40 for v in rng.integers(-2 ** 62, 2 ** 62, big_n)]          # beyond 64 bits: Python integers
    want = [s * v for v in S.y_part(t, n)]
    assert S.sub_sum(t, n) == want
    for radix in (2, 4, max(s, 2), 0):
        assert S.sub_sum_staged(t, n, radix) == want, radix
    # the automorphisms of SubSum fix every X^(s k)
    mono = [0] * big_n
    mono[s] = 1
    for i in range(s):
        assert S.rotate(mono, n * i) == mono


def test_sub_sum_stages():
    assert S.sub_sum_stages(512, 512) == [] and S.sub_sum_steps(512, 512) == []
    assert S.sub_sum_stages(512, 64, 2) == [[64], [128], [256]]
    assert S.sub_sum_stages(512, 64, 4) == [[64, 128, 192], [256]] == S.sub_sum_stages(512, 64)
    assert S.sub_sum_stages(512, 64, 8) == [[64 * i for i in range(1, 8)]] == S.sub_sum_stages(512, 64, 512)
    assert S.sub_sum_stages(8192, 256, 4) == [[256, 512, 768], [1024, 2048, 3072], [4096]]
    assert S.sub_sum_steps(512, 256, 4) == [256]
    for bad in ((512, 1, 4), (512, 3, 4), (512, 1024, 4), (512, 64, 3), (512, 64, 1)):
        with pytest.raises(AssertionError):
            S.sub_sum_stages(*bad)


@pytest.mark.parametrize("n,groups", [(64, [3, 3]), (256, [4, 4])])
def test_the_pipeline_returns_the_message(O, n, groups):
    """t = D p(Y) + q0 I(X) with I dense over all N coefficients; the bound is tests/test_bootstrap_spec.py's"""
    big_n, delta = 1024, float(1 << 50)
    primes = O.coeff_modulus_create(big_n, [60] + [50] * 17 + [60])[:-1]
    q0 = float(primes[0])
    tables = E.numpy_tables(10)
    s = big_n // (2 * n)
    rng = np.random.default_rng(n)
    p = np.zeros(big_n)
    p[::s] = rng.uniform(-1.0, 1.0, 2 * n)
    integers = rng.integers(-(K - 1), K, big_n).astype(np.float64)
    integers[:4] = [K - 1, -(K - 1), 0, K - 1]
    got, k = S.pipeline(delta * p + q0 * integers, n, primes, delta, K, DEGREE, DOUBLE_ANGLES, groups, groups, float(1 << 50), tables)
    assert k["levels"] == len(groups) + 10 + len(groups)
    e = B.interpolant_error(K, DEGREE, DOUBLE_ANGLES)
    bound = 4.0 * (6.58 * (delta / q0) ** 2 * 1.0 + e * 2 ** DOUBLE_ANGLES * (q0 / delta))
    err = float(np.max(np.abs(got - p)))
    print("n = %d: pipeline error %.3e, bound %.3e" % (n, err, bound))
    assert err <= bound
