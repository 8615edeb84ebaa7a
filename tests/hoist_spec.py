"""Exact big-integer SPECIFICATION of the hoisted rotations (troyn_apply_galois_many / troyn_apply_galois_sum, include/troyn.h) -- test
infrastructure, written as mathematics on Python integers with the pieces of tests/ks_spec.py (negacyclic products by Kronecker
substitution, the one rounded division by the special prime).

Per item, with the ciphertext (c0, c1) in coefficient form:
  * d_j = limb j of c1, integers in [0, q_j)
  * sigma_g on an integer polynomial: (sigma_g x)[i * g mod N] = (-1)^floor(i * g / N) x[i]
  * e_{t,j} = sigma_{g_t}(d_j): SIGNED coefficients in (-q_j, q_j) -- the decomposition happens before the automorphism
  * for every key modulus m in {q_0 .. q_{L-1}, q_special} and component c
        X_c[m] = SUM_{t in S} SUM_j (e_{t,j} mod m) (*) k_{t,j}[c][m]   mod m
  * r_c = the representative of X_c[q_special] in [-h, q_special - 1 - h], h = floor(q_special / 2)
  * result_c[l] = (X_c[q_l] - r_c) * q_special^-1 mod q_l
  * out[0][l] = SUM_{t in S} sigma_{g_t}(c0)[l] + result_0[l] mod q_l,   out[1][l] = result_1[l]
many: S = {t} for every t;  sum: S = all terms."""
from ks_spec import negacyclic


def sigma(x, g):
    """the automorphism X -> X^g on a polynomial with integer (signed) coefficients"""
    n = len(x)
    out = [0] * n
    for i, v in enumerate(x):
        r = i * g
        out[r % n] = -int(v) if (r // n) & 1 else int(v)
    return out


def inner_products(q, L, c1, elements, keys_coeff, automorphism=sigma):
    """P[t][c][k][i] = SUM_j (e_{t,j} mod q[k]) (*) k_{t,j}[c][q[k]] mod q[k] for k in {0 .. L-1, K-1} (None on the rows a level does not use)"""
    K = len(q)
    n = len(c1[0])
    P = []
    for t, g in enumerate(elements):
        e = [automorphism([int(v) for v in c1[j]], g) for j in range(L)]
        Pt = [[None] * K for _ in range(2)]
        for c in range(2):
            for k in list(range(L)) + [K - 1]:
                m = q[k]
                acc = [0] * n
                for j in range(L):
                    prod = negacyclic([v % m for v in e[j]], keys_coeff[t][j][c][k], m)
                    acc = [(x + y) % m for x, y in zip(acc, prod)]
                Pt[c][k] = acc
        P.append(Pt)
    return P


def finish(q, L, c0, elements, P, S, automorphism=sigma):
    """the rounded division by the special prime of SUM_{t in S} P[t] and the permuted c0: out[2][L][N] in coefficient form"""
    K = len(q)
    qs = q[K - 1]
    h = qs // 2
    n = len(c0[0])

    def X(c, k):
        acc = [0] * n
        for t in S:
            acc = [(x + y) % q[k] for x, y in zip(acc, P[t][c][k])]
        return acc

    out = [[None] * L for _ in range(2)]
    for c in range(2):
        r = [((v + h) % qs) - h for v in X(c, K - 1)]
        for l in range(L):
            inv = pow(qs, -1, q[l])
            res = [((x - rr) * inv) % q[l] for x, rr in zip(X(c, l), r)]
            if c == 0:
                for t in S:
                    res = [(a + b) % q[l] for a, b in zip(res, automorphism([int(v) for v in c0[l]], elements[t]))]
            out[c][l] = res
    return out


def apply_galois_sum_spec(q, L, c0, c1, elements, keys_coeff, automorphism=sigma):
    """q: the K key-level moduli (special prime last); c0, c1 [L][N] canonical, coefficient form; elements: the g_t of S;
    keys_coeff[t][j][c][k][i]: key of term t, digit j, component c, under modulus q[k], coefficient form.
    Returns out[2][L][N] in coefficient form.  `automorphism` exists for the specification's own tests (the identity map)."""
    P = inner_products(q, L, c1, elements, keys_coeff, automorphism)
    return finish(q, L, c0, elements, P, range(len(elements)), automorphism)


def apply_galois_many_spec(q, L, c0, c1, elements, keys_coeff):
    """one output per term: out[t][2][L][N]"""
    P = inner_products(q, L, c1, elements, keys_coeff)
    return [finish(q, L, c0, elements, P, [t]) for t in range(len(elements))]
