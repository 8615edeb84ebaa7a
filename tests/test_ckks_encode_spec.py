"""The numpy specification of the CKKS encoder (tests/ckks_encode_spec.py) against first principles, on the CPU."""
import numpy as np
import pytest

import ckks_encode_spec as S

LOG_N = 10
N = 1 << LOG_N


@pytest.fixture(scope="module")
def tables():
    return S.numpy_tables(LOG_N)


def test_index_map_is_the_generator_3_orbit(tables):
    index_map = tables[0]
    assert sorted(index_map.tolist()) == list(range(N))           # a permutation
    m = 2 * N
    for i in (0, 1, 2, 17, N // 2 - 1):
        e = pow(3, i, m)
        assert index_map[i] == S.reverse_bits((e - 1) // 2, LOG_N)
        assert index_map[i + N // 2] == S.reverse_bits((m - e - 1) // 2, LOG_N)


def test_encode_evaluates_to_the_values(tables):
    """the encoded polynomial, evaluated at psi^(3^i), gives back value i (before rounding): the transform is the canonical embedding"""
    rng = np.random.default_rng(5)
    vr, vi = rng.uniform(-1, 1, N // 2), rng.uniform(-1, 1, N // 2)
    c = S.simd_coefficients(vr, vi, 1.0, tables)
    for i in (0, 1, 5, N // 2 - 1):
        ang = 2.0 * np.pi * (pow(3, i, 2 * N) * np.arange(N) % (2 * N)) / (2 * N)
        z = np.sum(c * np.cos(ang)) + 1j * np.sum(c * np.sin(ang))
        assert abs(z - (vr[i] + 1j * vi[i])) < 1e-10


@pytest.mark.parametrize("seed,count,scale", [(1, N // 2, 2.0 ** 40), (2, 37, 2.0 ** 30), (3, N // 2, 2.0 ** 70)])
def test_round_trip_stays_inside_the_bound(O, tables, seed, count, scale):
    moduli = O.coeff_modulus_create(N, [60, 60, 40])
    rng = np.random.default_rng(seed)
    vr, vi = rng.uniform(-4, 4, count), rng.uniform(-4, 4, count)
    res, too_large = S.residues(S.simd_coefficients(vr, vi, scale, tables), moduli)
    assert not too_large
    gr, gi = S.simd_from_coefficients(S.polynomial_from_residues(res, moduli, scale), tables)
    bound = S.round_trip_bound(N, scale, np.sum(np.hypot(vr, vi)))
    full_r, full_i = np.zeros(N // 2), np.zeros(N // 2)
    full_r[:count], full_i[:count] = vr, vi
    err = np.max(np.hypot(gr - full_r, gi - full_i))
    print("round trip: max error %.3e, bound %.3e" % (err, bound))
    assert err <= bound


def test_residue_step_matches_the_oracle_ntt_of_hand_reduced_coefficients(O):
    """coefficients whose residues are known by hand, through the spec and through the oracle's transform pair"""
    moduli = O.coeff_modulus_create(N, [60, 40])
    coeffs = np.zeros(N)
    coeffs[0], coeffs[1], coeffs[2], coeffs[3], coeffs[4] = 5.0, -3.0, 2.5, 3.5, -(2.0 ** 70)      # 2.5 -> 2, 3.5 -> 4 (half to even)
    res, too_large = S.residues(coeffs, moduli)
    assert not too_large
    for i, q in enumerate(moduli):
        assert [int(x) for x in res[i][:5]] == [5, q - 3, 2, 4, (q - (1 << 70) % q) % q]
        assert not res[i][5:].any()
    tabs = [O.NTTTables(LOG_N, q) for q in moduli]
    ntt = O.ntt_forward(res.copy().reshape(-1), 1, len(moduli), LOG_N, tabs).reshape(len(moduli), N)
    # the transform of 5 - 3 X + 2 X^2 + 4 X^3 - 2^70 X^4 at the first root of the table: position 0 of the NTT holds the value at psi^bitrev(0)... = psi
    for i, q in enumerate(moduli):
        psi = tabs[i].root
        assert int(ntt[i][0]) == sum(int(res[i][j]) * pow(psi, j, q) for j in range(5)) % q
    back = O.ntt_inverse(ntt.copy().reshape(-1), 1, len(moduli), LOG_N, tabs).reshape(len(moduli), N)
    assert np.array_equal(back, res)
    assert S.residues(np.array([2.0 ** 128]), moduli)[1] and not S.residues(np.array([2.0 ** 127]), moduli)[1]


def test_compose_rounds_correctly(O):
    moduli = O.coeff_modulus_create(N, [60, 60])
    Q = moduli[0] * moduli[1]
    cases = [(1 << 53) + 1,            # tie -> even: 2^53
             (1 << 53) + 3,            # tie -> even: 2^53 + 4
             (1 << 54) + 2 + 1,        # above the tie: 2^54 + 4
             -((1 << 53) + 1), -((1 << 53) + 3), -5, 0, Q // 2, -(Q // 2),
             (1 << 117) + (1 << 64) + 1]       # the sticky bit lies words below the rounding position
    res = np.array([[x % q for x in cases] for q in moduli], dtype=np.uint64)
    assert S.compose(res, moduli) == cases
    got = S.polynomial_from_residues(res, moduli, 1.0)
    want = [2.0 ** 53, 2.0 ** 53 + 4, 2.0 ** 54 + 4, -(2.0 ** 53), -(2.0 ** 53 + 4), -5.0, 0.0, float(Q // 2), -float(Q // 2), 2.0 ** 117 + 2.0 ** 65]
    assert got.tolist() == want
    # Q/2 itself is not representable: (Q + 1) / 2 is Q - (Q - 1)/2, i.e. negative
    res2 = np.array([[(Q // 2 + 1) % q] for q in moduli], dtype=np.uint64)
    assert S.compose(res2, moduli) == [-(Q // 2)]
    assert S.polynomial_from_residues(res, moduli, 3.0).tolist() == [w / 3.0 for w in want]
