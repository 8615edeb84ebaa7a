"""The specification of the double-hoisted BSGS transform (tests/bsgs_double_spec.py) tied to what exists already, on the CPU:
  * one identity giant step: the words ARE those of the weighted sums with one slot (tests/weighted_hoist_spec.py);
  * reassociation: the per-row arithmetic equals the same sum formed over the CRT-composed integers modulo Q * q_special and ONE exact
    integer division, out = round_div( SUM_g [ sigma_G(X_0^(g)) + KS_G(v^(g)) ] );
  * with genuine Galois keys the output decrypts to the same message as tests/bsgs_spec.py's, within the sum of the two worst-case noise
    bounds, and the words differ."""
from fractions import Fraction

import numpy as np

from bsgs_double_spec import bsgs_double_spec, inner_values, key_rows
from bsgs_spec import bsgs_spec
from hoist_spec import sigma
from ks_spec import negacyclic
from test_bsgs_spec import BABIES, GIANTS, _genuine_keys, _plain_bsgs, _small_weights
from test_weighted_hoist_spec import _random_case
from weighted_hoist_spec import weighted_sums_spec

CASES = ((32, [50, 50, 50, 50], 3, False), (32, [50, 50, 50], 2, True))


def test_single_identity_giant_is_the_weighted_sum(O):
    for n, bits, L, reverse in CASES:
        q, c0, c1, keys, poly = _random_case(O, n, bits, L, 3, 17 + L, reverse)
        babies, bkeys = [1, 5, 2 * n - 1], [None, keys[0], keys[1]]
        w = lambda: [poly(m) for m in q]
        weights = [[w(), None, w()]]
        got = bsgs_double_spec(q, L, c0, c1, babies, bkeys, [1], [None], weights)
        for route in ("post", "pre"):
            assert [got] == weighted_sums_spec(q, L, c0, c1, babies, bkeys, weights, route), route


def _crt(q, rows, by_row):
    """the integers modulo the product of q[k], k in rows, from their residues by_row[k][i]"""
    M = 1
    for k in rows:
        M *= q[k]
    n = len(by_row[rows[0]])
    out = [0] * n
    for k in rows:
        Mk = M // q[k]
        f = Mk * pow(Mk, -1, q[k])
        out = [(a + f * int(b)) % M for a, b in zip(out, by_row[k])]
    return out, M


def test_reassociation_over_the_composed_integers(O):
    for n, bits, L, reverse in CASES:
        q, c0, c1, keys, poly = _random_case(O, n, bits, L, 4, 41 + L, reverse)
        K = len(q)
        qs, h = q[K - 1], q[K - 1] // 2
        rows = key_rows(q, L)
        babies, bkeys = [1, 5, 25], [None, keys[0], keys[1]]
        giants, gkeys = [125 % (2 * n), 1, 2 * n - 1], [keys[2], None, keys[3]]
        w = lambda: [poly(m) for m in q]
        weights = [[w(), w(), w()], [w(), None, w()], [None, w(), None]]
        got = bsgs_double_spec(q, L, c0, c1, babies, bkeys, giants, gkeys, weights)
        # the second way: every inner value as ONE integer polynomial modulo M = Q * q_special
        X = inner_values(q, L, c0, c1, babies, bkeys, weights)
        total = [[0] * n, [0] * n]
        M = None
        for g, G in enumerate(giants):
            x0, M = _crt(q, rows, X[g][0])
            x1, _ = _crt(q, rows, X[g][1])
            if G == 1:
                total[0] = [(a + b) % M for a, b in zip(total[0], x0)]
                total[1] = [(a + b) % M for a, b in zip(total[1], x1)]
                continue
            # v = the exact quotient (x1 - r) / q_special, an integer below Q in magnitude; its limbs are the digits
            r = [((v + h) % qs) - h for v in x1]
            assert all((a - b) % qs == 0 for a, b in zip(x1, r))
            v = [(a - b) // qs for a, b in zip(x1, r)]
            total[0] = [(a + b) % M for a, b in zip(total[0], sigma(x0, G))]
            for j in range(L):
                e = sigma([x % q[j] for x in v], G)
                for c in range(2):
                    kint, _ = _crt(q, rows, {k: gkeys[g][j][c][k] for k in rows})
                    total[c] = [(a + b) % M for a, b in zip(total[c], negacyclic([x % M for x in e], kint, M))]
        for c in range(2):
            r = [((v + h) % qs) - h for v in total[c]]
            assert all((a - b) % qs == 0 for a, b in zip(total[c], r))
            quotient = [(a - b) // qs for a, b in zip(total[c], r)]
            for l in range(L):
                assert got[c][l] == [x % q[l] for x in quotient], (c, l)


def test_genuine_keys_decrypt_like_the_single_hoisted_transform(O):
    """The CKKS-style ciphertext of tests/test_bsgs_spec.py (c0 + c1 * s = m + e, |e| <= E0 = 8, weights of magnitude W = 2, key noise
    |err| <= B = 21, ternary s).  With KS = L * N * B * q_max / q_special the noise a key switch leaves after the division, worst case:
      single-hoisted (derived there):  S = SUM_g [ inner(g) + (1 + N) / 2 ] + #{G != 1} KS + (1 + N) / 2
      double-hoisted:                  D = SUM_g inner(g) + #{G != 1} (KS + N / 2) + (1 + N) / 2
        inner(g) = SUM_{b in g} N W E0 + SUM_{b in g, B_b != 1} N W KS  -- the inner sums are not rounded; dividing only component 1 of a giant
        step with a key puts an error of at most 1/2 per coefficient on v, N / 2 in the phase v * s, which the giant key switch carries over
        (an automorphism keeps the norm) next to its own KS; the final division rounds both components, (1 + N) / 2.
    Both phases are within their bound of the same plaintext sum, so they differ by at most S + D.  The words are not equal."""
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
    args = (q, L, c0, c1, BABIES, bkeys, GIANTS, gkeys, weights)
    double, single = bsgs_double_spec(*args), bsgs_spec(*args)

    def phase(out):
        crt = lambda rows: [(rows[0][i] + q[0] * ((rows[1][i] - rows[0][i]) * pow(q[0], -1, q[1]) % q[1])) % Q for i in range(n)]
        p = [(a + b) % Q for a, b in zip(crt(out[0]), negacyclic(crt(out[1]), [v % Q for v in s], Q))]
        return [v - Q if v > Q // 2 else v for v in p]

    KS = Fraction(L * n * B * max(q[:L]), q[K - 1])
    half = Fraction(1 + n, 2)
    keyed_giants = sum(1 for g in GIANTS if g != 1)
    inner = sum(n * W * (E0 + (KS if b != 1 else 0)) for row in signed for b, w in zip(BABIES, row) if w is not None)
    S = inner + len(GIANTS) * half + keyed_giants * KS + half
    D = inner + keyed_giants * (KS + Fraction(n, 2)) + half
    want = _plain_bsgs(signed, message)
    pd, ps = phase(double), phase(single)
    worst_d = max(abs(a - b) for a, b in zip(pd, want))
    worst_s = max(abs(a - b) for a, b in zip(ps, want))
    apart = max(abs(a - b) for a, b in zip(pd, ps))
    print("double-hoisted spec: phase error %d (bound %d), single-hoisted %d (bound %d), apart %d" % (worst_d, D, worst_s, S, apart))
    assert worst_d <= D and worst_s <= S
    assert apart <= S + D
    assert max(abs(v) for v in want) > 1000 * (S + D)
    assert double != single
