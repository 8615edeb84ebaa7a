"""tests/packed_bootstrap_spec.py against the unpacked statements of tests/sparse_bootstrap_spec.py (CPU, float64): the packed table, the two identities of
troy/slot_transform.h "Packed", and the float64 chain t = D p(Y) + q0 I(X) -> p with ONE EvalMod operand.

  CoeffToSlot   P = v + conj(v), v = M1 u, against [2 Re(G u); 2 Im(G u)] of the unpacked group on n rows: bit for bit (the turned words give the same two
                products per term, the block's terms arrive in the same order, and x + x = 2 x is exact).
  SlotToCoeff   V + rot_n(V), V = F1 [a; b], against the unpacked group on a + i b: within 64 ulp of the largest output.  (F a and i F b are rounded before
                they are added, F (a + i b) adds inside every product: the two differ by roundings of the sums, at most 2^count terms of them.)
  pipeline      the bound of tests/test_sparse_bootstrap_spec.py, same parameters.
"""
import numpy as np
import pytest

import bootstrap_spec as B
import ckks_encode_spec as E
import dft_factors_spec as D
import packed_bootstrap_spec as P
import sparse_bootstrap_spec as S

CASES = [(64, 8), (1024, 4), (1024, 64), (1024, 256)]
K, DEGREE, DOUBLE_ANGLES = 64, 79, 3      # the choice of tests/test_gpu_bootstrap_api.py
_TABLES = {}


def _tables(big_n):
    if big_n not in _TABLES:
        _TABLES[big_n] = E.numpy_tables(D.log2_exact(big_n))
    return _TABLES[big_n]


def _counts(n):
    m = D.log2_exact(n)
    return sorted({1, m - 1, m})          # one layer, all but the top one, and blocks of n rows, which touch row n


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint64)


@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("big_n,n", CASES)
def test_the_table_is_the_sparse_table_on_2n_rows_with_the_lower_block_turned(big_n, n, inverse):
    tables = _tables(big_n)
    m = D.log2_exact(n)
    groups = {(0, c) for c in _counts(n)} | ({(1, m - 1)} if m >= 2 else set())
    for first, count in sorted(groups):
        for constant in (1.0, -0.7310585786300049):
            got = P.table(tables, n, first, count, inverse=inverse, constant=constant)
            base = S.table(tables, 2 * n, first, count, inverse=inverse, constant=constant)
            assert got.shape == base.shape == ((2 << count) - 1, 2 * n, 2) and P.diagonal_indices(n, first, count) == S.diagonal_indices(2 * n, first, count)
            assert np.array_equal(_bits(got[:, :n]), _bits(base[:, :n]))
            # the two blocks are identical, and the lower one is the upper one times -i / +i as complex numbers
            assert np.array_equal(_bits(base[:, n:]), _bits(base[:, :n]))
            upper, lower = got[:, :n, 0] + 1j * got[:, :n, 1], got[:, n:, 0] + 1j * got[:, n:, 1]
            assert np.array_equal(lower, upper * (-1j if inverse else 1j))
            # absent entries are +0 in both words; a present zero component is turned into -0.0 where the negation meets it
            absent = (base[:, n:, 0] == 0) & (base[:, n:, 1] == 0) & ~np.signbit(base[:, n:, 0]) & ~np.signbit(base[:, n:, 1])
            if count < m or first > 0:
                assert absent.any()
            assert not _bits(got[:, n:])[absent].any()
            negated = got[:, n:, 1] if inverse else got[:, n:, 0]
            source = base[:, n:, 0] if inverse else base[:, n:, 1]
            assert np.array_equal(np.signbit(negated)[~absent], ~np.signbit(source)[~absent])


def test_a_zero_component_becomes_minus_zero():
    """layer 0 forward from a unit constant: the entries of value 1 have an imaginary part +0, and +i times them is (-0.0, 1)"""
    tables = _tables(64)
    got, base = P.table(tables, 8, 0, 1), S.table(tables, 16, 0, 1)
    ones = (base[:, 8:, 0] == 1.0) & (base[:, 8:, 1] == 0.0)
    assert ones.any()
    assert np.all(got[:, 8:, 0][ones] == 0.0) and np.all(np.signbit(got[:, 8:, 0][ones])) and np.all(got[:, 8:, 1][ones] == 1.0)
    got = P.table(tables, 8, 0, 1, inverse=True, constant=2.0)          # (1, +0) -> (+0, -1)
    ones = (S.table(tables, 16, 0, 1, inverse=True, constant=2.0)[:, 8:, 0] == 1.0) & (S.table(tables, 16, 0, 1, inverse=True, constant=2.0)[:, 8:, 1] == 0.0)
    assert ones.any() and np.all(got[:, 8:, 1][ones] == -1.0) and not np.any(np.signbit(got[:, 8:, 0][ones]))


@pytest.mark.parametrize("big_n,n", CASES)
def test_coeff_to_slot_group_is_the_unpacked_group_bit_for_bit(big_n, n):
    tables = _tables(big_n)
    rng = np.random.default_rng(big_n + n)
    u_re, u_im = rng.uniform(-1, 1, n), rng.uniform(-1, 1, n)
    for count in _counts(n):
        for constant in (1.0, 0.37):
            p_re, p_im = P.coeff_to_slot_group(tables, n, count, u_re, u_im, constant)
            g_re, g_im = S.apply(S.table(tables, n, 0, count, inverse=True, constant=constant), n, 0, count, u_re, u_im)
            assert p_re.shape == (2 * n,) and not np.any(p_im)
            assert np.array_equal(_bits(p_re[:n]), _bits(2.0 * g_re)), (n, count)
            assert np.array_equal(_bits(p_re[n:]), _bits(2.0 * g_im)), (n, count)


@pytest.mark.parametrize("big_n,n", CASES)
def test_slot_to_coeff_group_is_the_unpacked_group_within_64_ulp(big_n, n):
    tables = _tables(big_n)
    rng = np.random.default_rng(3 * big_n + n)
    p = rng.uniform(-1, 1, 2 * n)
    for count in _counts(n):
        for constant in (1.0, 0.37):
            w_re, w_im = P.slot_to_coeff_group(tables, n, count, p, np.zeros(2 * n), constant)
            f_re, f_im = S.apply(S.table(tables, n, 0, count, constant=constant), n, 0, count, p[:n], p[n:])
            largest = max(float(np.max(np.abs(f_re))), float(np.max(np.abs(f_im))))
            err = max(float(np.max(np.abs(w_re - f_re))), float(np.max(np.abs(w_im - f_im))))
            print("N = %d n = %d count %d: |V + rot_n V - F (a + i b)| = %.3e = %.1f ulp of %.3e" % (big_n, n, count, err, err / np.spacing(largest), largest))
            assert err <= 64 * np.spacing(largest)


@pytest.mark.parametrize("n,groups", [(64, [3, 3]), (256, [4, 4])])
def test_whole_transforms_agree_with_the_unpacked_ones(n, groups):
    tables = _tables(1024)
    rng = np.random.default_rng(n)
    z_re, z_im = rng.uniform(-1, 1, n), rng.uniform(-1, 1, n)
    w_re, w_im = S.coeff_to_slot(tables, z_re, z_im, groups, 0.8)
    packed = P.coeff_to_slot(tables, z_re, z_im, groups, 0.8)
    assert np.array_equal(_bits(packed), _bits(np.concatenate([2.0 * w_re, 2.0 * w_im])))
    back = P.slot_to_coeff(tables, packed, groups, 1.0 / 1.6)
    assert max(float(np.max(np.abs(back[0] - z_re))), float(np.max(np.abs(back[1] - z_im)))) <= 8.0 * 10 * 2.0 ** -52 * n


@pytest.mark.parametrize("n,groups", [(64, [3, 3]), (256, [4, 4])])
def test_the_packed_pipeline_returns_the_message(O, n, groups):
    """the parameters, the message and the bound of tests/test_sparse_bootstrap_spec.py's pipeline test"""
    big_n, delta = 1024, float(1 << 50)
    primes = O.coeff_modulus_create(big_n, [60] + [50] * 17 + [60])[:-1]
    q0 = float(primes[0])
    tables = _tables(big_n)
    s = big_n // (2 * n)
    rng = np.random.default_rng(n)
    p = np.zeros(big_n)
    p[::s] = rng.uniform(-1.0, 1.0, 2 * n)
    integers = rng.integers(-(K - 1), K, big_n).astype(np.float64)
    integers[:4] = [K - 1, -(K - 1), 0, K - 1]
    t = delta * p + q0 * integers
    got, k = P.pipeline(t, n, primes, delta, K, DEGREE, DOUBLE_ANGLES, groups, groups, float(1 << 50), tables)
    assert k["levels"] == len(groups) + 10 + len(groups)
    e = B.interpolant_error(K, DEGREE, DOUBLE_ANGLES)
    bound = 4.0 * (6.58 * (delta / q0) ** 2 * 1.0 + e * 2 ** DOUBLE_ANGLES * (q0 / delta))
    err = float(np.max(np.abs(got - p)))
    unpacked, _ = S.pipeline(t, n, primes, delta, K, DEGREE, DOUBLE_ANGLES, groups, groups, float(1 << 50), tables)
    print("n = %d: packed pipeline error %.3e, unpacked %.3e, bound %.3e" % (n, err, float(np.max(np.abs(unpacked - p))), bound))
    assert err <= bound


def test_refusals():
    tables = _tables(64)
    for n, first, count in ((32, 0, 1), (1, 0, 1), (3, 0, 1), (8, 0, 4), (8, 2, 2), (8, 0, 0)):
        with pytest.raises(AssertionError):
            P.table(tables, n, first, count)
    with pytest.raises(AssertionError):
        P.coeff_to_slot(tables, np.zeros(8), np.zeros(8), [3], 1.0)
    with pytest.raises(AssertionError):
        P.slot_to_coeff(tables, np.zeros(16), [3], 1.0)
