"""Evaluator::multiply_affine_relinearize_rescale / evaluate_chebyshev / eval_mod (additions, troy/troy.h) through pytroy: payload against the
composition from the older methods, exact scales, decryption errors against float64 references and against the same schedule composed from
multiply_relinearize_rescale + linear_combination (bound: 4 x the composed form's error, measured in the same test), and the refusals."""
import numpy as np
import pytest
from numpy.polynomial import chebyshev as npcheb

import chebyshev_spec as S
from polyeval_spec import schedule
from test_gpu_hoist_api import _params, pytroy  # noqa: F401  (the module's fixture and parameter helper)

pytestmark = pytest.mark.gpu

N, BITS, WORK = 8192, [60] + [40] * 8 + [60], float(1 << 40)      # 9 data limbs: degree 31 takes 6 levels, eval_mod (15, r = 2) takes 7
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
        values = np.random.default_rng(2025).uniform(-1, 1, enc.slot_count())
        primes = [int(m.value()) for m in pytroy.CoeffModulus.create(N, BITS)][:-1]
        _STATE["ckks"] = (ctx, enc, kg.create_relin_keys(False), encryptor, pytroy.Decryptor(ctx, kg.secret_key()), pytroy.Evaluator(ctx), values, primes)
    return _STATE["ckks"]


def _encrypt(enc, encryptor, values, scale=WORK):
    return encryptor.encrypt_asymmetric_new(enc.encode_complex64_simd_new([complex(v) for v in values], None, scale))


def _decrypt(enc, dec, c):
    return np.asarray(enc.decode_complex64_simd_new(dec.decrypt_new(c))).real


def _lower(ev, c, limbs):
    while c.coeff_modulus_size() > limbs:
        c = ev.mod_switch_to_next_new(c)
    return c


def test_multiply_affine_relinearize_rescale(pytroy, dev):
    ctx, enc, rk, encryptor, dec, ev, values, primes = _setup(pytroy)
    rng = np.random.default_rng(7)
    xs = [values, rng.uniform(-1, 1, len(values)), rng.uniform(-1, 1, len(values))]
    a, b, c = [_encrypt(enc, encryptor, v) for v in xs]
    a, b = ev.mod_switch_to_next_new(a), ev.mod_switch_to_next_new(b)            # the addend sits one level above the operands
    L = a.coeff_modulus_size()
    assert c.coeff_modulus_size() == L + 1
    got = ev.multiply_affine_relinearize_rescale_new(a, b, 2, c, -1.0, 0.25, rk)
    S_prod = a.scale() * b.scale()
    assert got.scale() == S_prod / primes[L - 1]                                 # exactly
    assert got.coeff_modulus_size() == L - 1 and got.polynomial_count() == 2 and got.is_ntt_form()
    want = np.array(2 * xs[0] * xs[1] - xs[2] + 0.25)
    assert np.max(np.abs(_decrypt(enc, dec, got) - want)) < 2.0 ** -20
    # word for word: alpha = 1, no addend, no constant is the plain fused product
    plain = ev.multiply_affine_relinearize_rescale_new(a, b, 1, None, 0.0, 0.0, rk)
    assert plain.data() == ev.multiply_relinearize_rescale_new(a, b, rk).data()
    # ... and with the affine part the payload is the composition's: multiply; linear_combination of the product and the addend (carried on
    # three polynomials, the third zero), which weights the addend by -1 * (S / addend.scale) under the same rule; the constant 0.25 * S as a
    # plaintext; relinearize; rescale_to_next
    prod3 = ev.multiply_new(a, b)
    c3 = ev.sub_new(prod3, prod3)
    c3.set_scale(c.scale())
    c3 = ev.add_new(c3, _lower(ev, c, L))
    assert c3.polynomial_count() == 3
    lin = ev.linear_combination_new([prod3, c3], [2.0, -1.0], 0.0, S_prod)
    lin = ev.add_plain_new(lin, enc.encode_float64_single_new(0.25, lin.parms_id(), S_prod))
    comp = ev.rescale_to_next_new(ev.relinearize_new(lin, rk))
    assert comp.data() == got.data() and comp.scale() == got.scale()
    # keyword and batched forms
    dest = pytroy.Ciphertext()
    ev.multiply_affine_relinearize_rescale(encrypted1=a, encrypted2=b, alpha=2, addend=c, gamma=-1.0, constant=0.25, relin_keys=rk, destination=dest)
    assert dest.data() == got.data()
    d2 = [pytroy.Ciphertext(), pytroy.Ciphertext()]
    ev.multiply_affine_relinearize_rescale_batched(encrypted1=[a, a], encrypted2=[b, b], alpha=[2, 1], addend=[c, None], gamma=[-1.0, 0.0], constant=[0.25, 0.0],
                                                   relin_keys=rk, destination=d2)
    assert d2[0].data() == got.data() and d2[1].data() == plain.data()


def _composed_chebyshev(ev, enc, rk, x, coefficients, K, primes):
    """the same schedule from multiply_relinearize_rescale + linear_combination: every T_m is a product, rescaled, and THEN the affine part"""
    d = len(coefficients) - 1
    k, g, _, depth = schedule(d)
    u = S.leaf_coefficients(coefficients, d)
    y = x.clone()
    y.set_scale(x.scale() * K)
    L0, Sy = y.coeff_modulus_size(), y.scale()

    def leaf(ins, limbs, sum_scale, row):
        lc = ev.linear_combination_new([_lower(ev, c, limbs) for c in ins], [float(w) for w in row[1:]], 0.0, sum_scale)
        lc = ev.add_plain_new(lc, enc.encode_float64_single_new(float(row[0]), lc.parms_id(), sum_scale))      # (the constant at about 2^80 is beyond the sum's 62 bits)
        return ev.rescale_to_next_new(lc)

    if d <= 1:
        out = leaf([y], L0, Sy * primes[L0 - 1], u[0])
        out.set_scale(Sy)
        return out
    t = {1: y}
    for m in sorted(S.needed(d), key=lambda m: (S.depth_of(m), m)):
        a, b, r = S.split(m)
        limbs = min(t[a].coeff_modulus_size(), t[b].coeff_modulus_size())
        prod = ev.multiply_relinearize_rescale_new(_lower(ev, t[a], limbs), _lower(ev, t[b], limbs), rk)
        if r == 0:
            t[m] = ev.linear_combination_new([prod], [2.0], -1.0, prod.scale())
        else:
            t[m] = ev.linear_combination_new([prod, t[r]], [2.0, -1.0], 0.0, prod.scale())
    babies = [t[i] for i in range(1, k)]
    Lrec = L0 - (depth - 1)
    T = Sy * primes[Lrec - 1]
    total = None
    for j in range(1, g):
        G = _lower(ev, t[j * k], Lrec)
        term = ev.multiply_relinearize_rescale_new(leaf(babies, Lrec + 1, T / G.scale() * primes[Lrec], u[j]), G, rk)
        term.set_scale(Sy)
        total = term if total is None else ev.add_new(total, term)
    leaf0 = leaf(babies, Lrec, T, u[0])
    leaf0.set_scale(Sy)
    return ev.add_new(total, leaf0)


@pytest.mark.parametrize("K", [1, 4])
@pytest.mark.parametrize("d", [1, 7, 12, 31])
def test_evaluate_chebyshev(pytroy, dev, d, K):
    ctx, enc, rk, encryptor, dec, ev, values, primes = _setup(pytroy)
    coefficients = np.random.default_rng(100 + d).uniform(-1, 1, d + 1).tolist()
    xs = values * K                                                            # slots in [-K, K]; scale * K is the working scale 2^40
    x = _encrypt(enc, encryptor, xs, WORK / K)
    got = ev.evaluate_chebyshev_new(x, coefficients, float(K), rk)
    depth = schedule(d)[3]
    assert got.coeff_modulus_size() == x.coeff_modulus_size() - depth
    assert got.scale() == x.scale() * K and got.polynomial_count() == 2 and got.is_ntt_form()
    dest = pytroy.Ciphertext()
    ev.evaluate_chebyshev(encrypted=x, coefficients=coefficients, half_width=float(K), relin_keys=rk, destination=dest)
    assert dest.data() == got.data()
    want = npcheb.chebval(xs / K, coefficients)
    composed = _composed_chebyshev(ev, enc, rk, x, coefficients, K, primes)
    assert composed.coeff_modulus_size() == got.coeff_modulus_size()
    err_new = float(np.max(np.abs(_decrypt(enc, dec, got) - want)))
    err_old = float(np.max(np.abs(_decrypt(enc, dec, composed) - want)))
    print("evaluate_chebyshev d=%d K=%d: error %.3e, composed form %.3e, max|p| %.3e" % (d, K, err_new, err_old, float(np.max(np.abs(want)))))
    assert err_old < 2.0 ** -10 * float(np.max(np.abs(want)))                  # the ratio below must not hide a failure of both
    assert err_new <= 4 * err_old


def _interpolant(K, degree, r):
    """the Chebyshev interpolant of cos(2 pi (K y - 1/4) / 2^r) on [-1, 1] from the degree + 1 Chebyshev nodes, float64"""
    n = degree + 1
    nodes = np.cos(np.pi * (np.arange(n) + 0.5) / n)
    f = np.cos(2 * np.pi * (K * nodes - 0.25) / 2 ** r)
    c = np.array([2.0 / n * np.sum(f * np.cos(np.pi * j * (np.arange(n) + 0.5) / n)) for j in range(n)])
    c[0] /= 2
    return c


def test_eval_mod(pytroy, dev):
    ctx, enc, rk, encryptor, dec, ev, values, primes = _setup(pytroy)
    K, degree, r = 4, 15, 2
    rng = np.random.default_rng(15)
    m = rng.uniform(-2.0 ** -7, 2.0 ** -7, enc.slot_count())
    I = rng.integers(-3, 4, enc.slot_count())
    xs = m + I
    x = _encrypt(enc, encryptor, xs, WORK / K)
    got = ev.eval_mod_new(x, rk, float(K), degree, r)
    depth = schedule(degree)[3] + r
    assert got.coeff_modulus_size() == x.coeff_modulus_size() - depth
    dest = pytroy.Ciphertext()
    ev.eval_mod(encrypted=x, relin_keys=rk, half_width=float(K), degree=degree, double_angles=r, destination=dest)
    assert dest.data() == got.data()
    # reference 1: the same interpolant and doublings in float64
    coeffs = _interpolant(K, degree, r)
    v = npcheb.chebval(xs / K, coeffs)
    for _ in range(r):
        v = 2 * v * v - 1
    ref = v / (2 * np.pi)
    # the composed form: the composed Chebyshev schedule, then each doubling as a product, a rescale, and THEN 2 p - 1
    comp = _composed_chebyshev(ev, enc, rk, x, list(coeffs), K, primes)
    for _ in range(r):
        prod = ev.multiply_relinearize_rescale_new(comp, comp, rk)
        comp = ev.linear_combination_new([prod], [2.0], -1.0, prod.scale())
    comp.set_scale(comp.scale() * 2 * np.pi)
    dec_new, dec_old = _decrypt(enc, dec, got), _decrypt(enc, dec, comp)
    err_new, err_old = float(np.max(np.abs(dec_new - ref))), float(np.max(np.abs(dec_old - ref)))
    # reference 2: m itself; the bound is the interpolant's own distance from m (float64) plus the measured decryption error
    model = float(np.max(np.abs(ref - m)))
    err_m = float(np.max(np.abs(dec_new - m)))
    print("eval_mod degree %d r=%d K=%d: error vs interpolant %.3e, composed form %.3e; interpolant vs m %.3e, decryption vs m %.3e" %
          (degree, r, K, err_new, err_old, model, err_m))
    assert err_old < 2.0 ** -10
    assert err_new <= 4 * err_old
    assert err_m <= model + err_new
    # ... and that distance is bounded without the evaluation: sin(2 pi m) / (2 pi) - m is at most (2 pi)^2 |m|^3 / 6, and the interpolant's
    # error E against the cosine itself (a dense grid, float64) grows by at most 4 per doubling (|d(2v^2 - 1)/dv| <= 4 for |v| <= 1) before the
    # division by 2 pi.  A wrong interpolant, a wrong phase or a wrong 1 / (2 pi) on the device misses this bound by orders of magnitude.
    grid = np.linspace(-1, 1, 20001)
    E = float(np.max(np.abs(npcheb.chebval(grid, coeffs) - np.cos(2 * np.pi * (K * grid - 0.25) / 2 ** r))))
    bound = (2 * np.pi) ** 2 * (2.0 ** -7) ** 3 / 6 + 4 ** r * E / (2 * np.pi)
    print("eval_mod: interpolation error %.3e, bound on the distance from m %.3e" % (E, bound))
    assert model <= bound and err_m <= bound + 4 * err_old


def test_refusals(pytroy, dev):
    ctx, enc, rk, encryptor, dec, ev, values, primes = _setup(pytroy)
    x = _encrypt(enc, encryptor, values)
    coeff_form = ev.transform_from_ntt_new(x)
    for name, call in (("multiply_affine_relinearize_rescale", lambda c: ev.multiply_affine_relinearize_rescale_new(c, c, 2, None, 0.0, -1.0, rk)),
                       ("evaluate_chebyshev", lambda c: ev.evaluate_chebyshev_new(c, [1.0, 1.0, 1.0], 1.0, rk)),
                       ("eval_mod", lambda c: ev.eval_mod_new(c, rk, 4.0, 15, 2))):
        with pytest.raises(ValueError, match=r"%s\].*NTT" % name):               # coefficient form
            call(coeff_form)
    with pytest.raises(ValueError, match=r"evaluate_chebyshev\].*zero"):
        ev.evaluate_chebyshev_new(x, [0.0, 0.0, 0.0], 1.0, rk)
    with pytest.raises(ValueError, match=r"evaluate_chebyshev\].*127"):
        ev.evaluate_chebyshev_new(x, [0.0] * 128 + [1.0], 1.0, rk)
    with pytest.raises(ValueError, match=r"eval_mod\].*127"):
        ev.eval_mod_new(x, rk, 4.0, 128, 2)
    with pytest.raises(ValueError, match=r"evaluate_chebyshev\].*half width"):
        ev.evaluate_chebyshev_new(x, [1.0, 1.0], 0.0, rk)
    low = _lower(ev, x, 4)
    with pytest.raises(ValueError, match=r"evaluate_chebyshev\].*needs 5 limbs, the ciphertext has 4"):
        ev.evaluate_chebyshev_new(low, [1.0] * 8, 1.0, rk)                       # degree 7: depth 4
    with pytest.raises(ValueError, match=r"eval_mod\].*needs 8 limbs, the ciphertext has 4"):
        ev.eval_mod_new(low, rk, 4.0, 15, 2)                                     # depth 5 + 2
    last = _lower(ev, x, 1)
    with pytest.raises(ValueError, match=r"multiply_affine_relinearize_rescale\]"):      # no level left for the rescale
        ev.multiply_affine_relinearize_rescale_new(last, last, 2, None, 0.0, -1.0, rk)
    with pytest.raises(ValueError, match=r"multiply_affine_relinearize_rescale\].*alpha"):
        ev.multiply_affine_relinearize_rescale_new(x, x, 0, None, 0.0, -1.0, rk)
    with pytest.raises(ValueError, match=r"multiply_affine_relinearize_rescale\].*62 bits"):      # an addend weight of 2^62 or more
        ev.multiply_affine_relinearize_rescale_new(x, x, 2, x, 2.0 ** 22, 0.0, rk)    # S / addend.scale = 2^40
    with pytest.raises(ValueError, match=r"multiply_affine_relinearize_rescale\].*lower level"):
        ev.multiply_affine_relinearize_rescale_new(x, x, 2, ev.mod_switch_to_next_new(x), -1.0, 0.0, rk)
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
    bev, brk = pytroy.Evaluator(bctx), bkg.create_relin_keys(False)
    with pytest.raises(ValueError, match=r"multiply_affine_relinearize_rescale\].*CKKS only"):
        bev.multiply_affine_relinearize_rescale_new(bct, bct, 2, None, 0.0, -1.0, brk)
    with pytest.raises(ValueError, match=r"evaluate_chebyshev\].*CKKS only"):
        bev.evaluate_chebyshev_new(bct, [1.0, 2.0], 1.0, brk)
    with pytest.raises(ValueError, match=r"eval_mod\].*CKKS only"):
        bev.eval_mod_new(bct, brk, 4.0, 15, 2)
