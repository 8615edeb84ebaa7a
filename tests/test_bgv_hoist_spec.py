"""The specification of the hoisted BGV entries (tests/bgv_hoist_spec.py) tied to what exists already, on the CPU, on rings of N = 8 / 16
with three 20-bit primes and t = 17 / t = 2 (the plain modulus whose inverse of the special prime is 1):
  * adding the unkeyed contributions after the division, or injecting them before it scaled by the special prime, gives the same words;
  * bsgs is weighted_sums followed by sum_each; sum is weighted_sums with all-ones weights;
  * its division, fed plain (unpermuted) digits, gives the words of the oracle's BGV switch_key on the same keys;
  * with genuine Galois keys every output decrypts, through the oracle's BGV decryption, to the rotated / weighted plaintext modulo t."""
import numpy as np
import pytest

import bgv_hoist_spec as S
from hoist_spec import inner_products, sigma
from ks_spec import negacyclic

RINGS = ((8, 17), (16, 17), (16, 2), (8, 2))


def _case(O, n, terms, seed, L=2):
    q = [int(v) for v in O.coeff_modulus_create(n, [20, 20, 20])]
    assert all(m.bit_length() == 20 for m in q)
    K = len(q)
    rng = np.random.default_rng(seed)
    poly = lambda m: [int(v) for v in rng.integers(0, m, size=n, dtype=np.uint64)]
    c0 = [poly(q[l]) for l in range(L)]
    c1 = [poly(q[l]) for l in range(L)]
    keys = [[[[poly(q[k]) for k in range(K)] for c in range(2)] for j in range(L)] for _ in range(terms)]
    return q, c0, c1, keys, poly


@pytest.mark.parametrize("n,t", RINGS)
@pytest.mark.parametrize("L", [2, 1])
def test_pre_and_post_division_routes_give_the_same_words(O, n, t, L):
    q, c0, c1, keys, poly = _case(O, n, 4, 3 + n + t, L)
    elements = [5, 1, 2 * n - 1, 5]          # an identity term and a duplicate
    keys[1] = None
    w = lambda: [poly(m) for m in q]
    weights = [[w(), w(), w(), None], [None, w(), None, w()], [None, w(), None, None]]
    post = S.weighted_sums_spec(q, L, t, c0, c1, elements, keys, weights, "post")
    assert post == S.weighted_sums_spec(q, L, t, c0, c1, elements, keys, weights, "pre")
    assert post[0] != post[1]
    # a slot with the identity alone is the plain ciphertext-plaintext product of both components
    for c, src in enumerate((c0, c1)):
        for l in range(L):
            assert post[2][c][l] == negacyclic(weights[2][1][l], src[l], q[l])
    cts = [([poly(q[l]) for l in range(L)], [poly(q[l]) for l in range(L)]) for _ in elements]
    each = S.sum_each_spec(q, L, t, cts, elements, keys, "post")
    assert each == S.sum_each_spec(q, L, t, cts, elements, keys, "pre")
    args = (q, L, t, c0, c1, [1, 5, 2 * n - 1], [None, keys[0], keys[2]], elements, keys, [[w(), w(), None], [None, w(), None], [w(), None, w()], [w(), w(), w()]])
    assert S.bsgs_spec(*args, route="post") == S.bsgs_spec(*args, route="pre")


@pytest.mark.parametrize("n,t", RINGS)
def test_bsgs_is_weighted_sums_then_sum_each_and_sum_is_unit_weights(O, n, t):
    L = 2
    q, c0, c1, keys, poly = _case(O, n, 3, 11 + n + t)
    elements = [5, 3, 2 * n - 1]
    w = lambda: [poly(m) for m in q]
    weights = [[w(), None, w()], [w(), w(), w()]]
    giants, gkeys = [1, 3], [None, keys[1]]
    for route in ("post", "pre"):
        inner = S.weighted_sums_spec(q, L, t, c0, c1, elements, keys, weights, route)
        assert S.bsgs_spec(q, L, t, c0, c1, elements, keys, giants, gkeys, weights, route) == S.sum_each_spec(q, L, t, inner, giants, gkeys, route)
        one = [[1] + [0] * (n - 1) for _ in q]
        assert S.weighted_sums_spec(q, L, t, c0, c1, elements, keys, [[one, one, one]], route) == [S.sum_spec(q, L, t, c0, c1, elements, keys)]
    many = S.many_spec(q, L, t, c0, c1, elements, keys)
    assert len(many) == 3 and many[0] != many[1]
    assert S.many_spec(q, L, t, c0, c1, elements[:1], keys[:1])[0] == S.sum_spec(q, L, t, c0, c1, elements[:1], keys[:1])
    # the mod-t multiplier matters: the mutation the GPU tests must catch changes the words
    P = inner_products(q, L, c1, elements, keys)
    assert S.finish(q, L, t, c0, elements, P, range(3), multiplier=False) != S.finish(q, L, t, c0, elements, P, range(3))


@pytest.mark.parametrize("n,t", RINGS)
@pytest.mark.parametrize("L", [2, 1])
def test_division_on_plain_digits_is_the_oracles_bgv_switch_key(O, n, t, L):
    q = [int(v) for v in O.coeff_modulus_create(n, [20, 20, 20])]
    K = len(q)
    ctx = O.Context("bgv", n, q, t)
    keys_ntt = ctx.random_keys(5 + n, L)
    target_ntt = ctx.random_ct(9 + t, 1, L)[0]
    want = ctx.switch_key(L, True, target_ntt, keys_ntt)
    keys_c = [[[[int(v) for v in row] for row in ctx.from_ntt(kj[c][None], 1, K)[0]] for c in range(2)] for kj in keys_ntt]
    target_c = [[int(v) for v in row] for row in ctx.from_ntt(target_ntt[None], 1, L)[0]]
    P = inner_products(q, L, target_c, [3], [keys_c], automorphism=lambda x, g: x)[0]
    got = [S.divide(q, L, t, {k: P[c][k] for k in list(range(L)) + [K - 1]}) for c in range(2)]
    assert np.array_equal(ctx.to_ntt(np.array(got, dtype=np.uint64), 2, L), want)


def _coeff(ctx, x, pcount, rows):
    return [[[int(v) for v in row] for row in p] for p in ctx.from_ntt(np.asarray(x, dtype=np.uint64).reshape(pcount, rows, ctx.n), pcount, rows)]


@pytest.mark.parametrize("n,t", RINGS)
def test_genuine_keys_decrypt_exactly(O, n, t):
    q = [int(v) for v in O.coeff_modulus_create(n, [20, 20, 20])]
    K, L = len(q), len(q) - 1
    ctx = O.Context("bgv", n, q, t)
    rng = O.Rng(41 + n + t)
    sk = ctx.secret_key(rng)
    pk = ctx.public_key(rng, sk)
    prng = np.random.default_rng(n * t)
    message = [int(v) for v in prng.integers(0, t, size=n)]
    message[0] = 1
    ct = ctx.encrypt_asymmetric_bgv(rng, pk, np.array(message, dtype=np.uint64))
    assert [int(v) for v in ctx.decrypt_bgv(sk, ct)] == message
    elements = [3, 1, 2 * n - 1, 3]
    genuine = {g: _coeff(ctx, np.stack(ctx.galois_key(rng, sk, g)), L * 2, K) for g in (3, 2 * n - 1)}
    keys = [None if g == 1 else [[genuine[g][j * 2 + c] for c in range(2)] for j in range(L)] for g in elements]
    c0, c1 = _coeff(ctx, ct, 2, L)
    decrypt = lambda out: [int(v) for v in ctx.decrypt_bgv(sk, ctx.to_ntt(np.array(out, dtype=np.uint64), 2, L))]
    rot = lambda m, g: [v % t for v in sigma(m, g)]
    mul = lambda w, m: negacyclic([v % t for v in w], [v % t for v in m], t)
    addt = lambda a, b: [(x + y) % t for x, y in zip(a, b)]
    keyed = [0, 2, 3]
    # many / sum (no identity term)
    many = S.many_spec(q, L, t, c0, c1, [elements[u] for u in keyed], [keys[u] for u in keyed])
    total = [0] * n
    for out, u in zip(many, keyed):
        assert decrypt(out) == rot(message, elements[u])
        total = addt(total, rot(message, elements[u]))
    assert decrypt(S.sum_spec(q, L, t, c0, c1, [elements[u] for u in keyed], [keys[u] for u in keyed])) == total
    # weighted sums: small signed weights, one absent, centred into every key modulus
    signed = [[None if (s + u) % 5 == 4 else [int(v) for v in prng.integers(-2, 3, size=n)] for u in range(4)] for s in range(2)]
    weights = [[None if w is None else [[v % m for v in w] for m in q] for w in row] for row in signed]

    def inner_plain(row, m):
        acc = [0] * n
        for w, g in zip(row, elements):
            if w is not None:
                acc = addt(acc, mul(w, rot(m, g)))
        return acc

    for route in ("post", "pre"):
        inner = S.weighted_sums_spec(q, L, t, c0, c1, elements, keys, weights, route)
        for out, row in zip(inner, signed):
            assert decrypt(out) == inner_plain(row, message), route
        # sum_each over the two inner results, with an identity giant step; bsgs is the same thing
        giants, gkeys = [2 * n - 1, 1], [keys[2], None]
        want = addt(rot(inner_plain(signed[0], message), giants[0]), inner_plain(signed[1], message))
        assert decrypt(S.sum_each_spec(q, L, t, inner, giants, gkeys, route)) == want, route
        assert decrypt(S.bsgs_spec(q, L, t, c0, c1, elements, keys, giants, gkeys, weights, route)) == want, route
        assert any(want) or t == 2
