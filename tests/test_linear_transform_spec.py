"""The specification of LinearTransform against plain linear algebra (numpy only): the BSGS identity, the two device sources, the key list."""
import numpy as np
import pytest

import linear_transform_spec as S


def _complex(rng, *shape):
    return rng.uniform(-1, 1, shape) + 1j * rng.uniform(-1, 1, shape)


@pytest.mark.parametrize("n", [4, 16, 64])
def test_bsgs_identity(n):
    """SUM_G rot_G(SUM_B w[G][B] (.) rot_B(x)) = M x.  Both sides are sums of at most n products of numbers below sqrt(2) in modulus, added in different
    orders: they agree within n * 2 * 2^-52 * n, far above any rounding and far below a wrong index (errors of order 1)."""
    rng = np.random.default_rng(n)
    x = _complex(rng, n)
    tol = 2.0 * n * n * 2.0 ** -52
    M = _complex(rng, n, n)
    assert np.max(np.abs(S.bsgs_apply(S.diagonals_of(M), n, x) - M @ x)) <= tol
    # a sparse set with wrap-around indices: every other diagonal is zero
    keep = sorted({0, 1, 5 % n, n // 2, n - 1})
    d = S.diagonals_of(M)
    sparse = np.zeros_like(M)
    i = np.arange(n)
    for k in keep:
        sparse[i, (i + k) % n] = d[k]
    assert np.max(np.abs(S.bsgs_apply({k: d[k] for k in keep}, n, x) - sparse @ x)) <= tol
    # a baby count that is not the default
    other = 2 if S.default_baby_count(n) != 2 else 4
    assert np.max(np.abs(S.bsgs_apply(d, n, x, baby_count=other) - M @ x)) <= tol
    assert np.max(np.abs(S.bsgs_apply({k: d[k] for k in keep}, n, x, baby_count=n) - sparse @ x)) <= tol


@pytest.mark.parametrize("n,N", [(4, 8), (16, 32), (16, 256), (64, 1024)])
def test_matrix_mode_is_diagonals_mode(n, N):
    rng = np.random.default_rng(n + N)
    M = _complex(rng, n, n)
    d = S.diagonals_of(M)
    present = list(range(n))
    where_d, pd = S.pairs(present, n)
    where_m, pm = S.pairs(present, n, matrix=True)
    assert where_d == where_m and len(where_d) == n
    vd = S.values_of(np.stack([d[k] for k in present]), pd, n, N, False)
    vm = S.values_of(M, pm, n, N, True)
    assert vd.shape == (n, N // 2) and np.array_equal(vd, vm)
    # a short diagonal repeats across the slots
    assert np.array_equal(vd[:, :n], vd[:, N // 2 - n:])
    # a sparse table: a_t is the row of the table, not the diagonal index
    keep = [1, n - 1]
    _, pk = S.pairs(keep, n)
    _, pkm = S.pairs(keep, n, matrix=True)
    assert np.array_equal(S.values_of(np.stack([d[k] for k in keep]), pk, n, N, False), S.values_of(M, pkm, n, N, True))


def test_split_and_rotation_steps_of_a_fixed_example():
    present = [0, 1, 5, 8, 15]
    assert S.default_baby_count(16) == 4 and S.default_baby_count(8) == 4 and S.default_baby_count(4) == 2 and S.default_baby_count(1) == 1
    assert S.split(present, 16) == ([0, 1, 3], [0, 4, 8, 12])
    assert S.rotation_steps(present, 16) == [1, 3, 4, 8, 12]
    where, pr = S.pairs(present, 16)
    assert where == [(0, 0), (0, 1), (1, 1), (2, 0), (3, 2)]
    assert pr.tolist() == [[0, 0], [1, 0], [2, 4], [3, 8], [4, 12]]
    assert S.pairs(present, 16, matrix=True)[1].tolist() == [[0, 0], [1, 0], [5, 4], [8, 8], [15, 12]]
    assert S.split(present, 16, baby_count=8) == ([0, 1, 5, 7], [0, 8])
    assert S.rotation_steps(present, 16, baby_count=8) == [1, 5, 7, 8]
    assert S.rotation_steps(list(range(16)), 16, baby_count=4) == [1, 2, 3, 4, 8, 12]
    assert S.rotation_steps([0], 16) == []
