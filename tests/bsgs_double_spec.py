"""Exact big-integer SPECIFICATION of the double-hoisted baby-step/giant-step linear transform (troyn_linear_transform_bsgs_double_hoisted,
include/troyn.h) -- test infrastructure, mathematics on Python integers with the pieces of tests/ks_spec.py, tests/hoist_spec.py,
tests/weighted_hoist_spec.py and tests/bsgs_spec.py.

Per item, with the ciphertext (c0, c1) and the weights in coefficient form; rows = the key moduli {q_0 .. q_{L-1}, q_special}:
  * X^(g)_c[m] = the extended-basis value of weighted_hoist_spec for slot g on route "pre": the keyed products times their weights plus
    (q_special mod m) times the unkeyed contributions, nothing on the special row.  It is NOT divided.
  * G_g != 1:  v^(g)[l] = (X^(g)_1[q_l] - r) * q_special^-1 mod q_l, r the centred special row -- the only inner division, component 1 alone;
               Y_c[m] += hoist_spec.inner_products(v^(g), G_g, giant key)[c][m];   Y_0[m] += sigma_{G_g}(X^(g)_0[m]) mod m on every row
  * G_g  = 1:  Y_c[m] += X^(g)_c[m], both components
  * out_c[l] = (Y_c[q_l] - r_c) * q_special^-1 mod q_l."""
from hoist_spec import inner_products, sigma
from ks_spec import negacyclic
from weighted_hoist_spec import keyed_inner_products


def key_rows(q, L):
    return list(range(L)) + [len(q) - 1]


def inner_extended(q, L, c0, c1, elements, P, weights_s):
    """X[c][k] for k in key_rows: one slot of the weighted sums on the extended basis with the unkeyed contributions injected, undivided.
    weights_s[t] = rows [K] of coefficient-form weights or None; P from weighted_hoist_spec.keyed_inner_products."""
    K = len(q)
    qs = q[K - 1]
    n = len(c0[0])
    T = [t for t, w in enumerate(weights_s) if w is not None]
    assert T, "a giant step needs a weight"
    X = [dict(), dict()]
    for c in range(2):
        for k in key_rows(q, L):
            m = q[k]
            acc = [0] * n
            for t in T:
                if elements[t] != 1:
                    acc = [(x + y) % m for x, y in zip(acc, negacyclic(weights_s[t][k], P[t][c][k], m))]
                if k < L:
                    u = None
                    if c == 0:
                        u = [v % m for v in sigma([int(v) for v in c0[k]], elements[t])]
                    elif elements[t] == 1:
                        u = [int(v) for v in c1[k]]
                    if u is not None:
                        acc = [(x + (qs % m) * y) % m for x, y in zip(acc, negacyclic(weights_s[t][k], u, m))]
            X[c][k] = acc
    return X


def divide(q, L, X):
    """(X[q_l] - r) * q_special^-1 mod q_l with r the representative of X[q_special] in [-h, q_special - 1 - h]: [L][N]"""
    K = len(q)
    qs = q[K - 1]
    h = qs // 2
    r = [((v + h) % qs) - h for v in X[K - 1]]
    return [[((x - rr) * pow(qs, -1, q[l])) % q[l] for x, rr in zip(X[l], r)] for l in range(L)]


def outer_sum(q, L, X, giant_elements, giant_keys_coeff):
    """Y[c][k] from the inner values X[g][c][k]; also returns the v^(g) (None for the identity giant steps)"""
    n = len(X[0][0][0])
    rows = key_rows(q, L)
    Y = [{k: [0] * n for k in rows} for _ in range(2)]
    vs = []
    for g, G in enumerate(giant_elements):
        if G == 1:
            vs.append(None)
            for c in range(2):
                for k in rows:
                    Y[c][k] = [(a + b) % q[k] for a, b in zip(Y[c][k], X[g][c][k])]
            continue
        v = divide(q, L, X[g][1])
        vs.append(v)
        Pg = inner_products(q, L, v, [G], [giant_keys_coeff[g]])[0]
        for k in rows:
            m = q[k]
            for c in range(2):
                Y[c][k] = [(a + b) % m for a, b in zip(Y[c][k], Pg[c][k])]
            Y[0][k] = [(a + b) % m for a, b in zip(Y[0][k], sigma(X[g][0][k], G))]
    return Y, vs


def inner_values(q, L, c0, c1, baby_elements, baby_keys_coeff, weights):
    P = keyed_inner_products(q, L, c1, baby_elements, baby_keys_coeff)
    return [inner_extended(q, L, c0, c1, baby_elements, P, ws) for ws in weights]


def bsgs_double_spec(q, L, c0, c1, baby_elements, baby_keys_coeff, giant_elements, giant_keys_coeff, weights):
    """q: the K key-level moduli (special prime last); c0, c1 [L][N] canonical, coefficient form; weights[g][b]: [K][N] coefficient form or
    None, ALREADY rotated back by the giant step; keys as in hoist_spec (ignored for the element 1).  Returns out[2][L][N], coefficient form."""
    X = inner_values(q, L, c0, c1, baby_elements, baby_keys_coeff, weights)
    Y, _ = outer_sum(q, L, X, giant_elements, giant_keys_coeff)
    return [divide(q, L, Y[c]) for c in range(2)]
