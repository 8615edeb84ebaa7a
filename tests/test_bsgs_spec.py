"""The specification of the sum over different ciphertexts and of the baby-step/giant-step transform (tests/bsgs_spec.py) tied to what exists
already, on the CPU:
  * adding the unkeyed contributions after the division, or injecting them before it scaled by the special prime, gives the same words;
  * with every term the same ciphertext and no identity term it IS the specification of the summed form (tests/hoist_spec.py);
  * with only identity terms it is the plain sum;
  * with genuine Galois keys the BSGS output decrypts to SUM_g sigma_G( SUM_b w_{g,b} * sigma_B(m) ): exactly modulo t through the oracle's
    BFV decryption, and for a CKKS-style ciphertext (message + small error, no plain modulus) within the worst-case noise bound below."""
from fractions import Fraction

import numpy as np

from bsgs_spec import bsgs_spec, sum_each_spec
from hoist_spec import apply_galois_sum_spec, sigma
from ks_spec import negacyclic
from test_weighted_hoist_spec import _random_case

CASES = ((32, [50, 50, 50, 50], 3, False), (64, [60, 40, 40, 60], 3, False), (32, [50, 50, 50], 2, True))


def _cts(q, L, poly, terms):
    return [([poly(q[l]) for l in range(L)], [poly(q[l]) for l in range(L)]) for _ in range(terms)]


def test_pre_and_post_division_routes_give_the_same_words(O):
    for n, bits, L, reverse in CASES:
        q, _, _, keys, poly = _random_case(O, n, bits, L, 4, 31 + n, reverse)
        elements = [5, 25, 2 * n - 1, 1]
        keys[3] = None
        cts = _cts(q, L, poly, 4)
        post = sum_each_spec(q, L, cts, elements, keys, "post")
        assert post == sum_each_spec(q, L, cts, elements, keys, "pre")
        # ... and so does the composition
        w = lambda: [poly(m) for m in q]
        weights = [[w(), w(), None], [None, w(), None], [w(), None, w()], [w(), w(), w()]]
        args = (q, L, cts[0][0], cts[0][1], [1, 5, 25], [None, keys[0], keys[1]], elements, keys, weights)
        assert bsgs_spec(*args, route="post") == bsgs_spec(*args, route="pre")


def test_equal_inputs_without_identity_are_the_summed_form(O):
    for n, bits, L, reverse in CASES:
        q, c0, c1, keys, _ = _random_case(O, n, bits, L, 3, 7 + L, reverse)
        elements = [5, 25, 2 * n - 1]
        for route in ("post", "pre"):
            assert sum_each_spec(q, L, [(c0, c1)] * 3, elements, keys, route) == apply_galois_sum_spec(q, L, c0, c1, elements, keys), route


def test_identity_terms_alone_are_the_plain_sum(O):
    for n, bits, L, reverse in CASES:
        q, _, _, _, poly = _random_case(O, n, bits, L, 1, 3 + n, reverse)
        cts = _cts(q, L, poly, 3)
        want = [[[sum(ct[c][l][i] for ct in cts) % q[l] for i in range(n)] for l in range(L)] for c in range(2)]
        for route in ("post", "pre"):
            assert sum_each_spec(q, L, cts, [1, 1, 1], [None] * 3, route) == want, route


BABIES, GIANTS = [1, 3, 9], [1, 27, 63]      # N = 32: 63 = 2N - 1


def _genuine_keys(ctx, rng, sk, K, elements):
    """Galois keys of the oracle, in coefficient form under all K moduli (None for the identity)"""
    coeff = lambda kt: [[[[int(v) for v in row] for row in ctx.from_ntt(kj[c][None], 1, K)[0]] for c in range(2)] for kj in kt]
    return [None if g == 1 else coeff(ctx.galois_key(rng, sk, g)) for g in elements]


def _small_weights(q, seed):
    """signed weight polynomials in [-2, 2], one absent, one giant step with a single weight; centred into every key modulus"""
    wrng = np.random.default_rng(seed)
    signed = [[[int(v) for v in wrng.integers(-2, 3, size=32)] for _ in BABIES] for _ in GIANTS]
    signed[0][2] = None
    signed[2][0] = signed[2][1] = None
    return signed, [[None if w is None else [[v % m for v in w] for m in q] for w in row] for row in signed]


def _plain_bsgs(signed, message, modulus=None):
    """SUM_g sigma_G( SUM_b w_{g,b} * sigma_B(m) ) on integers (modulus None) or modulo `modulus`"""
    big = modulus or (1 << 200)
    centre = (lambda v: v) if modulus else (lambda v: v - big if v > big // 2 else v)
    total = [0] * len(message)
    for g, row in zip(GIANTS, signed):
        inner = [0] * len(message)
        for b, w in zip(BABIES, row):
            if w is not None:
                prod = negacyclic([v % big for v in w], [v % big for v in sigma(message, b)], big)
                inner = [x + centre(y) for x, y in zip(inner, prod)]
        total = [x + y for x, y in zip(total, sigma(inner, g))]
    return [v % modulus for v in total] if modulus else total


def test_genuine_keys_decrypt_to_the_bsgs_sum_bfv(O):
    n, t = 32, 257
    q = [int(v) for v in O.coeff_modulus_create(n, [36, 36, 37])]
    K, L = len(q), len(q) - 1
    ctx = O.Context("bfv", n, q, t)
    rng = O.Rng(29)
    sk = ctx.secret_key(rng)
    pk = ctx.public_key(rng, sk)
    ct = ctx.encrypt_asymmetric_bfv(rng, pk, ctx.batch_encode(list(range(1, n + 1))))
    message = [int(v) for v in ctx.decrypt_bfv(sk, ct)]
    bkeys, gkeys = _genuine_keys(ctx, rng, sk, K, BABIES), _genuine_keys(ctx, rng, sk, K, GIANTS)
    signed, weights = _small_weights(q, 4)
    c0 = [[int(v) for v in ct[0][l]] for l in range(L)]
    c1 = [[int(v) for v in ct[1][l]] for l in range(L)]
    got = np.array(bsgs_spec(q, L, c0, c1, BABIES, bkeys, GIANTS, gkeys, weights), dtype=np.uint64)
    want = _plain_bsgs(signed, message, t)
    assert [int(v) for v in ctx.decrypt_bfv(sk, got)] == want
    assert any(want)


def test_genuine_keys_decrypt_to_the_bsgs_sum_ckks(O):
    """A CKKS-style ciphertext on integers: c0 + c1 * s = m + e with |m| < 2^30 and |e| <= E0 = 8, no plain modulus.  The phase of the
    specification's output is compared with the plaintext BSGS sum on integers.  The bound is the worst case of the scheme, not a measurement
    (tests/test_hoist_spec.py checks its decryptions exactly and holds no CKKS bound to reuse, so it is derived here):
      * a key switch adds SUM_j e_j * err_j before the division, |e_j| < q_max the signed digits, |err_j| <= B = 21 the key noise (centred
        binomial): at most L * N * q_max * B, divided by the special prime P: KS = L * N * B * q_max / P;
      * a weight of magnitude W = 2 multiplies a polynomial's norm by at most N * W;
      * a rounded division adds at most 1/2 per component, (1 + N) / 2 in the phase (ternary s);
      inner(g) = SUM_{b in g} N W E0 + SUM_{b in g, B_b != 1} N W KS + (1 + N) / 2
      total    = SUM_g inner(g) + #{g : G_g != 1} KS + (1 + N) / 2         (an automorphism keeps the norm)."""
    n = 32
    q = [int(v) for v in O.coeff_modulus_create(n, [36, 36, 37])]
    K, L = len(q), len(q) - 1
    ctx = O.Context("ckks", n, q)
    rng = O.Rng(31)
    sk = ctx.secret_key(rng)
    s = [int(v) for v in ctx.from_ntt(sk[None], 1, K)[0][0]]
    s = [v - q[0] if v > q[0] // 2 else v for v in s]
    assert set(s) <= {-1, 0, 1} and any(s)
    prng = np.random.default_rng(6)
    E0, W, B = 8, 2, 21
    message = [int(v) for v in prng.integers(-(1 << 30), 1 << 30, size=n)]
    error = [int(v) for v in prng.integers(-E0, E0 + 1, size=n)]
    Q = q[0] * q[1]
    c1_int = [int(a) * int(b) % Q for a, b in zip(prng.integers(0, 1 << 62, size=n), prng.integers(0, 1 << 62, size=n))]
    c1s = negacyclic(c1_int, [v % Q for v in s], Q)
    c0_int = [(m + e - x) % Q for m, e, x in zip(message, error, c1s)]
    c0 = [[v % q[l] for v in c0_int] for l in range(L)]
    c1 = [[v % q[l] for v in c1_int] for l in range(L)]
    bkeys, gkeys = _genuine_keys(ctx, rng, sk, K, BABIES), _genuine_keys(ctx, rng, sk, K, GIANTS)
    signed, weights = _small_weights(q, 8)
    out = bsgs_spec(q, L, c0, c1, BABIES, bkeys, GIANTS, gkeys, weights)
    # the phase out0 + out1 * s, composed over q_0 q_1 and centred
    crt = lambda rows: [(rows[0][i] + q[0] * ((rows[1][i] - rows[0][i]) * pow(q[0], -1, q[1]) % q[1])) % Q for i in range(n)]
    o0, o1 = crt(out[0]), crt(out[1])
    phase = [(a + b) % Q for a, b in zip(o0, negacyclic(o1, [v % Q for v in s], Q))]
    phase = [v - Q if v > Q // 2 else v for v in phase]
    want = _plain_bsgs(signed, message)
    KS = Fraction(L * n * B * max(q[:L]), q[K - 1])
    half = Fraction(1 + n, 2)
    bound = half + sum(KS for g in GIANTS if g != 1)
    for row in signed:
        bound += half + sum(n * W * (E0 + (KS if b != 1 else 0)) for b, w in zip(BABIES, row) if w is not None)
    worst = max(abs(a - b) for a, b in zip(phase, want))
    print("ckks bsgs spec: worst phase error %d, bound %d, message magnitude %d" % (worst, bound, max(abs(v) for v in want)))
    assert worst <= bound
    assert max(abs(v) for v in want) > 1000 * bound
