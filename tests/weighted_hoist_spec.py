"""Exact big-integer SPECIFICATION of the plaintext-weighted hoisted rotations (troyn_apply_galois_weighted_sums, include/troyn.h) -- test
infrastructure, mathematics on Python integers with the pieces of tests/hoist_spec.py and tests/ks_spec.py.

Per item and slot s, with the ciphertext (c0, c1) in coefficient form and the weights in COEFFICIENT form (w[s][t][k] under key modulus q[k],
None = the term is absent from the slot; only the rows 0 .. L-1 and K-1 are used).  T_s = the terms present in slot s:
  * X_c[m]  = SUM_{t in T_s, g_t != 1} w_{s,t}[m] (*) P[t][c][m]  mod m     (P: hoist_spec.inner_products, one Barrett-reduced product per term)
  * y_0[l]  = SUM_{t in T_s}           w_{s,t}[q_l] (*) sigma_{g_t}(c0)[l]  mod q_l
    y_1[l]  = SUM_{t in T_s, g_t = 1}  w_{s,t}[q_l] (*) c1[l]               mod q_l         (the unkeyed contributions)
  * r_c     = the representative of X_c[q_special] in [-h, q_special - 1 - h], h = floor(q_special / 2)
  * route "post":  out[c][l] = (X_c[q_l] - r_c) * q_special^-1 + y_c[l]                          mod q_l
    route "pre":   out[c][l] = ((X_c[q_l] + (q_special mod q_l) * y_c[l]) - r_c) * q_special^-1  mod q_l
The two routes give the same words (tests/test_weighted_hoist_spec.py checks it); an implementation may take either."""
from hoist_spec import inner_products, sigma
from ks_spec import negacyclic


def keyed_inner_products(q, L, c1, elements, keys_coeff):
    """hoist_spec.inner_products for the terms with a key; None for the identity terms (their keys_coeff entry is not looked at)"""
    keyed = [t for t, g in enumerate(elements) if g != 1]
    Pk = inner_products(q, L, c1, [elements[t] for t in keyed], [keys_coeff[t] for t in keyed])
    P = [None] * len(elements)
    for i, t in enumerate(keyed):
        P[t] = Pk[i]
    return P


def finish_weighted(q, L, c0, c1, elements, P, weights_s, route="post"):
    """one slot: weights_s[t] = rows [K] of coefficient-form weights or None; P from keyed_inner_products.  Returns out[2][L][N], coefficient form."""
    K = len(q)
    qs = q[K - 1]
    h = qs // 2
    n = len(c0[0])
    T = [t for t, w in enumerate(weights_s) if w is not None]
    assert T, "a slot needs a weight"

    def add(a, b, m):
        return [(x + y) % m for x, y in zip(a, b)]

    out = [[None] * L for _ in range(2)]
    for c in range(2):
        X = {}
        for k in list(range(L)) + [K - 1]:
            acc = [0] * n
            for t in T:
                if elements[t] != 1:
                    acc = add(acc, negacyclic(weights_s[t][k], P[t][c][k], q[k]), q[k])
            X[k] = acc
        r = [((v + h) % qs) - h for v in X[K - 1]]
        for l in range(L):
            m = q[l]
            y = [0] * n
            for t in T:
                if c == 0:
                    y = add(y, negacyclic(weights_s[t][l], [v % m for v in sigma([int(v) for v in c0[l]], elements[t])], m), m)
                elif elements[t] == 1:
                    y = add(y, negacyclic(weights_s[t][l], [int(v) for v in c1[l]], m), m)
            inv = pow(qs, -1, m)
            if route == "post":
                out[c][l] = [((x - rr) * inv + yy) % m for x, rr, yy in zip(X[l], r, y)]
            else:
                scaled = [(x + (qs % m) * yy) % m for x, yy in zip(X[l], y)]
                out[c][l] = [((x - rr) * inv) % m for x, rr in zip(scaled, r)]
    return out


def weighted_sums_spec(q, L, c0, c1, elements, keys_coeff, weights, route="post"):
    """q: the K key-level moduli (special prime last); c0, c1 [L][N] canonical, coefficient form; elements: odd g_t < 2N, 1 = the identity;
    keys_coeff[t][j][c][k][i] as in hoist_spec (ignored for g_t = 1); weights[s][t]: [K][N] coefficient form or None.
    Returns out[slots][2][L][N] in coefficient form."""
    P = keyed_inner_products(q, L, c1, elements, keys_coeff)
    return [finish_weighted(q, L, c0, c1, elements, P, ws, route) for ws in weights]
