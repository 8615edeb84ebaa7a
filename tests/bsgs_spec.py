"""Exact big-integer SPECIFICATION of the sum over different ciphertexts (troyn_apply_galois_sum_each) and of the baby-step/giant-step linear
transform (troyn_linear_transform_bsgs, include/troyn.h) -- test infrastructure, mathematics on Python integers with the pieces of
tests/hoist_spec.py, tests/weighted_hoist_spec.py and tests/ks_spec.py.

sum_each, per item, with one ciphertext (c0_t, c1_t) PER TERM in coefficient form:
  * X_c[m]  = SUM_{t, g_t != 1} P_t[c][m]  mod m      (P_t: hoist_spec.inner_products of c1_t with the key of term t, one product per term)
  * y_0[l]  = SUM_t            sigma_{g_t}(c0_t)[l]  mod q_l
    y_1[l]  = SUM_{t, g_t = 1} c1_t[l]               mod q_l         (the unkeyed contributions)
  * r_c     = the representative of X_c[q_special] in [-h, q_special - 1 - h], h = floor(q_special / 2)
  * route "post":  out[c][l] = (X_c[q_l] - r_c) * q_special^-1 + y_c[l]                          mod q_l
    route "pre":   out[c][l] = ((X_c[q_l] + (q_special mod q_l) * y_c[l]) - r_c) * q_special^-1  mod q_l
bsgs: weighted_sums_spec over the baby steps with one slot per giant step, then sum_each over those results with the giant steps."""
from hoist_spec import inner_products, sigma
from weighted_hoist_spec import weighted_sums_spec


def each_inner_products(q, L, cts, elements, keys_coeff):
    """P[t] = hoist_spec.inner_products of c1 of term t with the key of term t; None for the identity terms"""
    return [None if g == 1 else inner_products(q, L, cts[t][1], [g], [keys_coeff[t]])[0] for t, g in enumerate(elements)]


def sum_each_spec(q, L, cts, elements, keys_coeff, route="post", P=None):
    """q: the K key-level moduli (special prime last); cts[t] = (c0, c1), each [L][N] canonical, coefficient form; elements: odd g_t < 2N,
    1 = the identity; keys_coeff[t][j][c][k][i] as in hoist_spec (ignored for g_t = 1); P: each_inner_products, when the caller has them.
    Returns out[2][L][N] in coefficient form."""
    K = len(q)
    qs = q[K - 1]
    h = qs // 2
    n = len(cts[0][0][0])
    rows = list(range(L)) + [K - 1]
    if P is None:
        P = each_inner_products(q, L, cts, elements, keys_coeff)
    out = [[None] * L for _ in range(2)]
    for c in range(2):
        X = {k: [0] * n for k in rows}
        for t, g in enumerate(elements):
            if g != 1:
                for k in rows:
                    X[k] = [(x + y) % q[k] for x, y in zip(X[k], P[t][c][k])]
        r = [((v + h) % qs) - h for v in X[K - 1]]
        for l in range(L):
            m = q[l]
            y = [0] * n
            for t, g in enumerate(elements):
                if c == 0:
                    y = [(a + b) % m for a, b in zip(y, sigma([int(v) for v in cts[t][0][l]], g))]
                elif g == 1:
                    y = [(a + int(b)) % m for a, b in zip(y, cts[t][1][l])]
            inv = pow(qs, -1, m)
            if route == "post":
                out[c][l] = [((x - rr) * inv + yy) % m for x, rr, yy in zip(X[l], r, y)]
            else:
                scaled = [(x + (qs % m) * yy) % m for x, yy in zip(X[l], y)]
                out[c][l] = [((x - rr) * inv) % m for x, rr in zip(scaled, r)]
    return out


def bsgs_spec(q, L, c0, c1, baby_elements, baby_keys_coeff, giant_elements, giant_keys_coeff, weights, route="post"):
    """weights[g][b]: [K][N] coefficient form or None, ALREADY rotated back by the giant step.  Returns out[2][L][N] in coefficient form."""
    inner = weighted_sums_spec(q, L, c0, c1, baby_elements, baby_keys_coeff, weights, route)
    return sum_each_spec(q, L, inner, giant_elements, giant_keys_coeff, route)
