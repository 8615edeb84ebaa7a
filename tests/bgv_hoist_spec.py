"""Exact big-integer SPECIFICATION of the hoisted BGV entries (troyn_bgv_apply_galois_many / _sum / _weighted_sums / _sum_each and
troyn_bgv_linear_transform_bsgs, include/troyn.h) -- test infrastructure, mathematics on Python integers.  Everything before the division
is that of the BFV/CKKS entries and is imported from their specifications; the division by the special prime qk is BGV's (ski_util5):
  * s_c         = X_c[qk] in coefficient form, canonical
  * dk_l(s)     = [-s qk^-1 mod t]_{q_l} qk + [s]_{q_l}  mod q_l           (bgv_chain_spec.delta)
  * route "post":  out[c][l] = (X_c[q_l] - dk_l(s_c)) qk^-1 + y_c[l]                       mod q_l
    route "pre":   out[c][l] = ((X_c[q_l] + (qk mod q_l) y_c[l]) - dk_l(s_c)) qk^-1        mod q_l
with y the unkeyed contributions of each entry.  dk depends on the special row alone, so the two routes give the same words
(tests/test_bgv_hoist_spec.py checks it).  All polynomials are in coefficient form; the correction is linear, so subtracting it there is
subtracting its transform from the NTT-form words."""
from bgv_chain_spec import delta
from bsgs_spec import each_inner_products
from hoist_spec import inner_products, sigma
from ks_spec import negacyclic
from weighted_hoist_spec import keyed_inner_products


def _add(a, b, m):
    return [(x + y) % m for x, y in zip(a, b)]


def divide(q, L, t, X, y=None, route="post", multiplier=True):
    """X: {k: row} for k in 0 .. L-1 and K-1, coefficient form; y: [L] rows of unkeyed contributions or None.  Returns [L][N].
    multiplier=False drops the mod-t multiplier k (the mutation the GPU tests must catch)."""
    K = len(q)
    qk = q[K - 1]
    inv_t = pow(qk, -1, t) if multiplier else 0
    s = [v % qk for v in X[K - 1]]
    out = []
    for l in range(L):
        m = q[l]
        inv = pow(qk, -1, m)
        d = delta(s, qk, inv_t, t, m)
        yl = y[l] if y is not None else [0] * len(s)
        if route == "post":
            out.append([((x - dd) * inv + yy) % m for x, dd, yy in zip(X[l], d, yl)])
        else:
            scaled = [(x + (qk % m) * yy) % m for x, yy in zip(X[l], yl)]
            out.append([((x - dd) * inv) % m for x, dd in zip(scaled, d)])
    return out


def _rows(q, L):
    return list(range(L)) + [len(q) - 1]


def finish(q, L, t, c0, elements, P, S, **kw):
    """many / sum: the BGV division of SUM_{t in S} P[t] and the permuted c0 added after it.  P: hoist_spec.inner_products.  out[2][L][N]"""
    n = len(c0[0])
    out = []
    for c in range(2):
        X = {}
        for k in _rows(q, L):
            acc = [0] * n
            for u in S:
                acc = _add(acc, P[u][c][k], q[k])
            X[k] = acc
        y = None
        if c == 0:
            y = []
            for l in range(L):
                acc = [0] * n
                for u in S:
                    acc = _add(acc, sigma([int(v) for v in c0[l]], elements[u]), q[l])
                y.append(acc)
        out.append(divide(q, L, t, X, y, "post", **kw))
    return out


def sum_spec(q, L, t, c0, c1, elements, keys_coeff):
    P = inner_products(q, L, c1, elements, keys_coeff)
    return finish(q, L, t, c0, elements, P, range(len(elements)))


def many_spec(q, L, t, c0, c1, elements, keys_coeff):
    P = inner_products(q, L, c1, elements, keys_coeff)
    return [finish(q, L, t, c0, elements, P, [u]) for u in range(len(elements))]


def finish_weighted(q, L, t, c0, c1, elements, P, weights_s, route="post", **kw):
    """one slot of weighted_sums: weights_s[u] = rows [K] of coefficient-form weights or None; P: keyed_inner_products.  out[2][L][N]"""
    n = len(c0[0])
    T = [u for u, w in enumerate(weights_s) if w is not None]
    assert T, "a slot needs a weight"
    out = []
    for c in range(2):
        X = {}
        for k in _rows(q, L):
            acc = [0] * n
            for u in T:
                if elements[u] != 1:
                    acc = _add(acc, negacyclic(weights_s[u][k], P[u][c][k], q[k]), q[k])
            X[k] = acc
        y = []
        for l in range(L):
            m = q[l]
            acc = [0] * n
            for u in T:
                if c == 0:
                    acc = _add(acc, negacyclic(weights_s[u][l], [v % m for v in sigma([int(v) for v in c0[l]], elements[u])], m), m)
                elif elements[u] == 1:
                    acc = _add(acc, negacyclic(weights_s[u][l], [int(v) for v in c1[l]], m), m)
            y.append(acc)
        out.append(divide(q, L, t, X, y, route, **kw))
    return out


def weighted_sums_spec(q, L, t, c0, c1, elements, keys_coeff, weights, route="post", **kw):
    """weights[s][u]: [K][N] coefficient form or None.  Returns out[slots][2][L][N]"""
    P = keyed_inner_products(q, L, c1, elements, keys_coeff)
    return [finish_weighted(q, L, t, c0, c1, elements, P, ws, route, **kw) for ws in weights]


def sum_each_spec(q, L, t, cts, elements, keys_coeff, route="post", P=None, **kw):
    """cts[u] = (c0, c1), one ciphertext per term.  Returns out[2][L][N]"""
    n = len(cts[0][0][0])
    if P is None:
        P = each_inner_products(q, L, cts, elements, keys_coeff)
    out = []
    for c in range(2):
        X = {k: [0] * n for k in _rows(q, L)}
        for u, g in enumerate(elements):
            if g != 1:
                for k in X:
                    X[k] = _add(X[k], P[u][c][k], q[k])
        y = []
        for l in range(L):
            acc = [0] * n
            for u, g in enumerate(elements):
                if c == 0:
                    acc = _add(acc, sigma([int(v) for v in cts[u][0][l]], g), q[l])
                elif g == 1:
                    acc = _add(acc, [int(v) for v in cts[u][1][l]], q[l])
            y.append(acc)
        out.append(divide(q, L, t, X, y, route, **kw))
    return out


def bsgs_spec(q, L, t, c0, c1, baby_elements, baby_keys_coeff, giant_elements, giant_keys_coeff, weights, route="post", **kw):
    """weights[g][b]: [K][N] coefficient form or None, ALREADY rotated back by the giant step.  Returns out[2][L][N]"""
    inner = weighted_sums_spec(q, L, t, c0, c1, baby_elements, baby_keys_coeff, weights, route, **kw)
    return sum_each_spec(q, L, t, inner, giant_elements, giant_keys_coeff, route, **kw)
