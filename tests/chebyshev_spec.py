"""The contract of troyn_ckks_multiply_affine_relinearize_rescale (include/troyn.h) up to its relinearize, in Python big integers, and the
Chebyshev schedule built on that step: the ladder T_m = 2 T_a T_(m-a) - T_|2a-m|, the leaf coefficients of the Paterson-Stockmeyer
recombination in the Chebyshev basis, and the depth formula (the k and g of tests/polyeval_spec.py).

  P_0 = alpha (a0 . b0) + w c0 + k      P_1 = alpha (a0 . b1 + a1 . b0) + w c1      P_2 = alpha (a1 . b1)      mod q_l, canonical form

a, b are [2][L][N], c is [2][>= L][N] or None, alpha, w, k are [L] canonical residues (k may be None).
"""
import numpy as np

from polyeval_spec import clog2, schedule


def _big(x):
    return np.asarray(x, dtype=np.uint64).astype(object)


def step_direct(moduli, a, b, c, alpha, w, k):
    """the formula as it stands: ONE reduction per word, after the whole expression over the integers -> uint64 [3][L][N]"""
    L, n = len(moduli), a.shape[-1]
    out = np.zeros((3, L, n), dtype=np.uint64)
    for l, q in enumerate(moduli):
        a0, a1, b0, b1 = _big(a[0, l]), _big(a[1, l]), _big(b[0, l]), _big(b[1, l])
        p = [int(alpha[l]) * (a0 * b0), int(alpha[l]) * (a0 * b1 + a1 * b0), int(alpha[l]) * (a1 * b1)]
        if c is not None:
            p[0] = p[0] + int(w[l]) * _big(c[0, l])
            p[1] = p[1] + int(w[l]) * _big(c[1, l])
        if k is not None:
            p[0] = p[0] + int(k[l])
        for j in range(3):
            out[j, l] = (p[j] % int(q)).astype(np.uint64)
    return out


# -- the older operations, each with its own reduction ------------------------------------------------------------------------------
def dyadic_convolute(moduli, a, b):
    """troyn_dyadic_convolute for two-polynomial operands: every product reduced, sums by add_mod"""
    L, n = len(moduli), a.shape[-1]
    out = np.zeros((3, L, n), dtype=object)
    for l, q in enumerate(moduli):
        q = int(q)
        a0, a1, b0, b1 = _big(a[0, l]), _big(a[1, l]), _big(b[0, l]), _big(b[1, l])
        out[0, l] = (a0 * b0) % q
        out[1, l] = ((a0 * b1) % q + (a1 * b0) % q) % q
        out[2, l] = (a1 * b1) % q
    return out


def multiply_scalar(moduli, x, s):
    """troyn_multiply_scalar limb by limb: x [p][L][N], s [L]"""
    out = np.zeros(x.shape, dtype=object)
    for l, q in enumerate(moduli):
        out[:, l] = (x[:, l] * int(s[l])) % int(q)
    return out


def add(moduli, x, y):
    out = np.zeros(x.shape, dtype=object)
    for l, q in enumerate(moduli):
        out[:, l] = (x[:, l] + y[:, l]) % int(q)
    return out


def step_fold(moduli, a, b, c, alpha, w, k):
    """the same words from the fold of the older operations: convolute, multiply_scalar by alpha, multiply_scalar and add of the addend
    (its first L limbs), the constant at every index of polynomial 0"""
    L = len(moduli)
    p = multiply_scalar(moduli, dyadic_convolute(moduli, a, b), alpha)
    if c is not None:
        wc = multiply_scalar(moduli, _big(c[:, :L]), w)
        p[:2] = add(moduli, p[:2], wc)
    if k is not None:
        const = np.zeros((1, L, a.shape[-1]), dtype=object)
        for l in range(L):
            const[0, l, :] = int(k[l])
        p[:1] = add(moduli, p[:1], const)
    return p.astype(np.uint64)


# -- the Chebyshev schedule ---------------------------------------------------------------------------------------------------------
MAX_DEGREE = 127


def split(m):
    """T_m = 2 T_a T_(m-a) - T_(2a-m): a power of two is the double angle of T_(m/2) (the addend is T_0 = 1, a constant), any other m
    takes the largest power of two below m.  -> (a, m - a, 2a - m)"""
    a = 1
    while a * 2 < m:
        a *= 2
    return a, m - a, 2 * a - m


def needed(d):
    """every T_m with m > 1 the schedule computes: the babies 2..k-1, the giants jk, and what their recurrences pull in"""
    k, g, _, _ = schedule(d)
    want = set(range(2, k)) | ({k} | {j * k for j in range(1, g)} if d > 1 else set())
    todo = sorted(want)
    while todo:
        m = todo.pop()
        for r in split(m):
            if r > 1 and r not in want:
                want.add(r)
                todo.append(r)
    return want


def depth_of(m):
    """levels below the input at which T_m sits"""
    return clog2(m)


def total_depth(d):
    """as stated for evaluate_polynomial: max(ceil(log2((g-1)k)), log2 k + 1) + 1, and 1 for d <= 1"""
    return schedule(d)[3]


def ladder(y, d):
    """{m: T_m(y)} in float64 by the recurrence alone, every T_m one step; all T_m of one depth form one batch -> (values, batches)"""
    t = {0: np.ones_like(y), 1: y}
    batches = {}
    for m in sorted(needed(d)):
        batches.setdefault(depth_of(m), []).append(m)
    for dep in sorted(batches):
        for m in batches[dep]:
            a, b, r = split(m)
            assert max(depth_of(a), depth_of(b)) == dep - 1 and (r == 0 or depth_of(r) <= dep - 1)      # operands exist one level up
            t[m] = 2.0 * t[a] * t[b] - t[r]
    return t, batches


def leaf_coefficients(coefficients, d):
    """u[j][i] with p = SUM_j (SUM_i u[j][i] T_i) T_(jk), from T_i T_(jk) = (T_(jk+i) + T_(jk-i)) / 2, solved from the top block down"""
    k, g, _, _ = schedule(d)
    if d <= 1:
        return [[float(coefficients[i]) if i <= d else 0.0 for i in range(2)]]
    r = [float(coefficients[m]) if m <= d else 0.0 for m in range(g * k)]
    u = [[0.0] * k for _ in range(g)]
    for j in range(g - 1, 0, -1):
        u[j][0] = r[j * k]
        for i in range(1, k):
            u[j][i] = 2.0 * r[j * k + i]
            r[j * k - i] -= r[j * k + i]      # the mirror image T_(jk-i) that the product brings along
    u[0] = r[:k]
    return u


def evaluate(y, coefficients):
    """p(y) = SUM_m coefficients[m] T_m(y) by the schedule, float64"""
    d = len(coefficients)
    while d and coefficients[d - 1] == 0:
        d -= 1
    if d == 0:
        raise ValueError("all coefficients are zero")
    d -= 1
    if d > MAX_DEGREE:
        raise ValueError("degree above %d" % MAX_DEGREE)
    u = leaf_coefficients(coefficients, d)
    if d <= 1:
        return u[0][0] + u[0][1] * y
    k, g, _, _ = schedule(d)
    t, _ = ladder(y, d)
    leaf = lambda row: sum(row[i] * t[i] for i in range(k))
    return leaf(u[0]) + sum(leaf(u[j]) * t[j * k] for j in range(1, g))
