"""Evaluator::linear_combinations / linear_combination / evaluate_polynomial (additions: scalar-weighted sums of ciphertexts in one pass, and
polynomial evaluation on the fixed Paterson-Stockmeyer schedule of troy/troy.h) through pytroy: levels, scales, decryptions against the
float values and against the same schedule composed from the older Evaluator methods, and the refusals."""
import numpy as np
import pytest

import polyeval_spec as S
from test_gpu_hoist_api import _params, pytroy  # noqa: F401  (the module's fixture and parameter helper)

pytestmark = pytest.mark.gpu

N, BITS, SCALE = 8192, [60, 40, 40, 40, 40, 40, 40, 60], float(1 << 40)
_STATE = {}


def _setup(pytroy):
    if "ckks" not in _STATE:
        p = _params(pytroy, pytroy.SchemeType.CKKS, N, BITS)
        ctx = pytroy.HeContext(p, True, pytroy.SecurityLevel.Nil, 31)
        ctx.to_device_inplace()
        enc = pytroy.CKKSEncoder(ctx)
        kg = pytroy.KeyGenerator(ctx)
        encryptor = pytroy.Encryptor(ctx)
        encryptor.set_public_key(kg.create_public_key(False))
        rng = np.random.default_rng(2024)
        values = rng.uniform(-1, 1, enc.slot_count())
        primes = [int(m.value()) for m in pytroy.CoeffModulus.create(N, BITS)][:-1]
        _STATE["ckks"] = (ctx, enc, kg.create_relin_keys(False), encryptor, pytroy.Decryptor(ctx, kg.secret_key()), pytroy.Evaluator(ctx), values, primes)
    return _STATE["ckks"]


def _encrypt(enc, encryptor, values):
    return encryptor.encrypt_asymmetric_new(enc.encode_complex64_simd_new([complex(v) for v in values], None, SCALE))


def _decrypt(enc, dec, c):
    return np.asarray(enc.decode_complex64_simd_new(dec.decrypt_new(c))).real


def test_linear_combinations(pytroy, dev):
    ctx, enc, rk, encryptor, dec, ev, values, primes = _setup(pytroy)
    rng = np.random.default_rng(5)
    xs = [values, rng.uniform(-1, 1, len(values)), rng.uniform(-1, 1, len(values))]
    cts = [_encrypt(enc, encryptor, v) for v in xs]
    cts[2] = ev.mod_switch_to_next_new(cts[2])                    # two different levels
    assert cts[2].coeff_modulus_size() == cts[0].coeff_modulus_size() - 1
    weights = [[0.75, -0.5, 0.25], [-1.0, 0.0, 0.3333]]
    constants = [0.125, -2.5]
    scale = float(1 << 60)                                        # weights as integers of 20 bits, constants below 2^62
    got = ev.linear_combinations_new(cts, weights, constants, scale)
    assert len(got) == 2
    for s, c in enumerate(got):
        assert c.coeff_modulus_size() == cts[2].coeff_modulus_size() and c.parms_id() == cts[2].parms_id()      # the lowest level
        assert c.scale() == scale and c.is_ntt_form() and c.polynomial_count() == 2
        want = sum(w * x for w, x in zip(weights[s], xs)) + constants[s]
        # weights are rounded to multiples of 2^-20 (three of them, |x| <= 1); fresh encryption noise at scale 2^40 is orders below
        assert np.max(np.abs(_decrypt(enc, dec, c) - want)) < 3 * 2.0 ** -21 + 1e-6
    one = ev.linear_combination_new(cts, weights[1], constants[1], scale)
    assert one.data() == got[1].data() and one.scale() == scale
    dest = [pytroy.Ciphertext(), pytroy.Ciphertext()]
    ev.linear_combinations(encrypted=cts, weights=weights, constants=constants, scale=scale, destination=dest)
    assert [d.data() for d in dest] == [g.data() for g in got]
    d1 = pytroy.Ciphertext()
    ev.linear_combination(encrypted=cts, weights=weights[0], constant=constants[0], scale=scale, destination=d1)
    assert d1.data() == got[0].data()
    # refusals, each with the method's name
    with pytest.raises(ValueError, match=r"linear_combinations\].*Empty"):
        ev.linear_combinations_new([], weights, constants, scale)
    with pytest.raises(ValueError, match=r"linear_combinations\].*weight row"):
        ev.linear_combinations_new(cts, [[1.0, 2.0]], [0.0], scale)
    with pytest.raises(ValueError, match=r"linear_combination\].*weight row"):
        ev.linear_combination_new(cts, [1.0], 0.0, scale)
    with pytest.raises(ValueError, match=r"linear_combinations\].*NTT form"):
        ev.linear_combinations_new([ev.transform_from_ntt_new(cts[0])], [[1.0]], [0.0], scale)
    with pytest.raises(ValueError, match=r"linear_combinations\].*62 bits"):
        ev.linear_combinations_new(cts, weights, [8.0, 0.0], scale)
    with pytest.raises(ValueError, match=r"linear_combinations\].*polynomial counts"):
        ev.linear_combinations_new([cts[0], ev.multiply_new(cts[0], cts[1])], [[1.0, 1.0]], [0.0], scale)


def _composed(ev, enc, rk, x, coefficients, primes):
    """the same schedule through the older methods: powers by multiply_relinearize_rescale, leaves term by term with encode_float64_single +
    multiply_plain + add, the recombination per giant with multiply_relinearize_rescale + add"""
    d = S.degree(coefficients)
    k, g, needed, depth = S.schedule(d)
    L0, Sx = x.coeff_modulus_size(), x.scale()
    coef = lambda m: float(coefficients[m]) if m <= d else 0.0

    def lower(c, limbs):
        while c.coeff_modulus_size() > limbs:
            c = ev.mod_switch_to_next_new(c)
        return c

    def leaf(ins, limbs, sum_scale, cs):
        acc = None
        for c, w in zip(ins, cs[1:]):
            if w == 0.0:
                continue
            c = lower(c, limbs)
            t = ev.multiply_plain_new(c, enc.encode_float64_single_new(w, c.parms_id(), sum_scale / c.scale()))
            t.set_scale(sum_scale)                                 # (the product's scale differs from sum_scale in the last bits)
            acc = t if acc is None else ev.add_new(acc, t)
        if acc is None:
            return None
        acc = ev.add_plain_new(acc, enc.encode_float64_single_new(cs[0], acc.parms_id(), sum_scale))
        return ev.rescale_to_next_new(acc)

    if d <= 1:
        out = leaf([x], L0, Sx * primes[L0 - 1], [coef(0), coef(1)])
        out.set_scale(Sx)
        return out
    memo = {1: x}

    def power(m):
        if m not in memo:
            a, b = S.split(m)
            pa, pb = power(a), power(b)
            limbs = min(pa.coeff_modulus_size(), pb.coeff_modulus_size())
            memo[m] = ev.multiply_relinearize_rescale_new(lower(pa, limbs), lower(pb, limbs), rk)
        return memo[m]

    babies = [power(i) for i in range(1, k)]
    Lrec = L0 - (depth - 1)
    T = Sx * primes[Lrec - 1]
    total = None
    for j in range(1, g):
        G = lower(power(j * k), Lrec)
        cs = [coef(j * k + i) for i in range(k)]
        lf = leaf(babies, Lrec + 1, T / G.scale() * primes[Lrec], cs)
        if lf is None:                                             # a leaf that is its constant alone
            term = ev.rescale_to_next_new(ev.multiply_plain_new(G, enc.encode_float64_single_new(cs[0], G.parms_id(), T / G.scale())))
        else:
            term = ev.multiply_relinearize_rescale_new(lf, G, rk)
        term.set_scale(Sx)
        total = term if total is None else ev.add_new(total, term)
    leaf0 = leaf(babies, Lrec, T, [coef(i) for i in range(k)])
    if leaf0 is None:
        leaf0_plain = enc.encode_float64_single_new(coef(0), total.parms_id(), Sx)
        return ev.add_plain_new(total, leaf0_plain)
    leaf0.set_scale(Sx)
    return ev.add_new(total, leaf0)


@pytest.mark.parametrize("d", [1, 2, 7, 12])
def test_evaluate_polynomial(pytroy, dev, d):
    ctx, enc, rk, encryptor, dec, ev, values, primes = _setup(pytroy)
    coefficients = np.random.default_rng(100 + d).uniform(-1, 1, d + 1).tolist()
    x = _encrypt(enc, encryptor, values)
    got = ev.evaluate_polynomial_new(x, coefficients, rk)
    depth = S.schedule(d)[3]
    assert got.coeff_modulus_size() == x.coeff_modulus_size() - depth          # the fixed schedule, not Horner's d levels
    assert got.scale() == x.scale() and got.polynomial_count() == 2 and got.is_ntt_form()
    dest = pytroy.Ciphertext()
    ev.evaluate_polynomial(encrypted=x, coefficients=coefficients, relin_keys=rk, destination=dest)
    assert dest.data() == got.data()
    want = np.polyval(coefficients[::-1], values)
    composed = _composed(ev, enc, rk, x, coefficients, primes)
    assert composed.coeff_modulus_size() == got.coeff_modulus_size()
    err_new = float(np.max(np.abs(_decrypt(enc, dec, got) - want)))
    err_old = float(np.max(np.abs(_decrypt(enc, dec, composed) - want)))
    print("evaluate_polynomial d=%d: error %.3e, composed form %.3e, max|p| %.3e" % (d, err_new, err_old, float(np.max(np.abs(want)))))
    assert err_old < 2.0 ** -10 * float(np.max(np.abs(want)))                  # the ratio below must not hide a failure of both
    assert err_new <= 4 * err_old                                              # two forms that differ only in where roundings fall


def test_evaluate_polynomial_refusals(pytroy, dev):
    ctx, enc, rk, encryptor, dec, ev, values, primes = _setup(pytroy)
    x = _encrypt(enc, encryptor, values)
    with pytest.raises(ValueError, match=r"evaluate_polynomial\].*zero"):
        ev.evaluate_polynomial_new(x, [0.0, 0.0, 0.0], rk)
    with pytest.raises(ValueError, match=r"evaluate_polynomial\].*zero"):
        ev.evaluate_polynomial_new(x, [], rk)
    with pytest.raises(ValueError, match=r"evaluate_polynomial\].*NTT form"):
        ev.evaluate_polynomial_new(ev.transform_from_ntt_new(x), [1.0, 1.0], rk)
    low = x
    while low.coeff_modulus_size() > 4:
        low = ev.mod_switch_to_next_new(low)
    with pytest.raises(ValueError, match=r"evaluate_polynomial\].*needs 5 limbs, the ciphertext has 4"):
        ev.evaluate_polynomial_new(low, [1.0] * 8, rk)                          # degree 7: depth 4
    # a BFV context
    p = _params(pytroy, pytroy.SchemeType.BFV, 4096, [36, 36, 37])
    bctx = pytroy.HeContext(p, True, pytroy.SecurityLevel.Nil, 3)
    bctx.to_device_inplace()
    benc = pytroy.BatchEncoder(bctx)
    benc.to_device_inplace()
    bkg = pytroy.KeyGenerator(bctx)
    bencryptor = pytroy.Encryptor(bctx)
    bencryptor.set_public_key(bkg.create_public_key(False))
    bct = bencryptor.encrypt_asymmetric_new(benc.encode_simd_new([1, 2, 3]))
    bev = pytroy.Evaluator(bctx)
    with pytest.raises(ValueError, match=r"evaluate_polynomial\].*CKKS only"):
        bev.evaluate_polynomial_new(bct, [1.0, 2.0], bkg.create_relin_keys(False))
    with pytest.raises(ValueError, match=r"linear_combinations\].*CKKS only"):
        bev.linear_combinations_new([bct], [[1.0]], [0.0], 1.0)
