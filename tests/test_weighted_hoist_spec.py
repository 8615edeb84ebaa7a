"""The specification of the plaintext-weighted hoisted rotations (tests/weighted_hoist_spec.py) tied to what exists already, on the CPU:
  * with every weight the constant 1 and no identity term it IS the specification of the summed form (tests/hoist_spec.py);
  * adding the unkeyed contributions after the division, or injecting them before it scaled by the special prime, gives the same words;
  * with genuine Galois keys its output decrypts, through the oracle's BFV decryption, to SUM_t w_t * sigma_t(m) modulo t."""
import numpy as np

from hoist_spec import apply_galois_sum_spec
from ks_spec import negacyclic
from weighted_hoist_spec import weighted_sums_spec


def _random_case(O, n, bits, L, terms, seed, reverse=False):
    q = [int(v) for v in O.coeff_modulus_create(n, bits)]
    if reverse:
        q = sorted(q, reverse=True)
    K = len(q)
    rng = np.random.default_rng(seed)
    poly = lambda m: [int(v) for v in rng.integers(0, m, size=n, dtype=np.uint64)]
    c0 = [poly(q[l]) for l in range(L)]
    c1 = [poly(q[l]) for l in range(L)]
    keys = [[[[poly(q[k]) for k in range(K)] for c in range(2)] for j in range(L)] for t in range(terms)]
    return q, c0, c1, keys, poly


def test_unit_weights_are_the_summed_form(O):
    for n, bits, L, reverse in ((32, [50, 50, 50, 50], 3, False), (32, [50, 50, 50], 2, True)):
        q, c0, c1, keys, _ = _random_case(O, n, bits, L, 3, 5 + L, reverse)
        elements = [5, 25, 2 * n - 1]
        one = [[1] + [0] * (n - 1) for _ in q]
        for route in ("post", "pre"):
            got = weighted_sums_spec(q, L, c0, c1, elements, keys, [[one, one, one]], route)
            assert got == [apply_galois_sum_spec(q, L, c0, c1, elements, keys)], route


def test_pre_and_post_division_routes_give_the_same_words(O):
    for n, bits, L, reverse in ((32, [50, 50, 50, 50], 3, False), (64, [60, 40, 40, 60], 3, False), (32, [50, 50, 50], 2, True), (16, [30, 30], 1, False)):
        q, c0, c1, keys, poly = _random_case(O, n, bits, L, 4, 11 + n, reverse)
        elements = [5, 1, 2 * n - 1, 1]          # two identity terms, one of them only in slot 1
        keys[1] = keys[3] = None
        w = lambda: [poly(m) for m in q]
        weights = [[w(), w(), w(), None], [None, None, w(), w()], [None, w(), None, None]]
        post = weighted_sums_spec(q, L, c0, c1, elements, keys, weights, "post")
        pre = weighted_sums_spec(q, L, c0, c1, elements, keys, weights, "pre")
        assert post == pre
        assert len(post) == 3 and post[0] != post[1]
        # a slot with the identity alone is the plain ciphertext-plaintext product of both components
        for c, src in enumerate((c0, c1)):
            for l in range(L):
                assert post[2][c][l] == negacyclic(weights[2][1][l], src[l], q[l])


def test_genuine_keys_decrypt_to_the_weighted_sum(O):
    n, t = 32, 257
    q = [int(v) for v in O.coeff_modulus_create(n, [36, 36, 37])]
    K, L = len(q), len(q) - 1
    ctx = O.Context("bfv", n, q, t)
    rng = O.Rng(23)
    sk = ctx.secret_key(rng)
    pk = ctx.public_key(rng, sk)
    ct = ctx.encrypt_asymmetric_bfv(rng, pk, ctx.batch_encode(list(range(1, n + 1))))
    elements = [3, 1, 2 * n - 1]
    keys_ntt = [None if g == 1 else ctx.galois_key(rng, sk, g) for g in elements]
    keys_c = [None if kt is None else [[[[int(v) for v in row] for row in ctx.from_ntt(kj[c][None], 1, K)[0]] for c in range(2)] for kj in kt] for kt in keys_ntt]
    # the plaintexts sigma_t(m) as the oracle's own apply_galois decrypts them (polynomials modulo t); the identity: the ciphertext itself
    rotated = [ctx.decrypt_bfv(sk, ct if g == 1 else ctx.apply_galois_ct(L, False, g, ct, keys_ntt[i])) for i, g in enumerate(elements)]
    # small signed weight polynomials, centred into every key modulus (what transform_plain_to_ntt's centralize does before the transform)
    wrng = np.random.default_rng(2)
    signed = [[int(v) for v in wrng.integers(-2, 3, size=n)] for _ in elements]
    weights = [[[[v % m for v in w] for m in q] for w in signed]]
    c0 = [[int(v) for v in ct[0][l]] for l in range(L)]
    c1 = [[int(v) for v in ct[1][l]] for l in range(L)]
    got = np.array(weighted_sums_spec(q, L, c0, c1, elements, keys_c, weights)[0], dtype=np.uint64)
    want = [0] * n
    for w, m in zip(signed, rotated):
        want = [(a + b) % t for a, b in zip(want, negacyclic([v % t for v in w], [int(v) for v in m], t))]
    assert [int(v) for v in ctx.decrypt_bfv(sk, got)] == want
    assert any(want)
