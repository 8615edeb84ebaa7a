"""Integer specification of the fused BGV chain (troyn_bgv_multiply_relinearize_mod_switch) on a tiny ring, in Python integers.

Two independent restatements:
  composed(...)  the three steps one after the other, each as its own stand-alone entry computes it: the tensor product, the BGV
                 relinearization (key-switch inner product, mod-t correction of the special prime, division) and the BGV modulus switch
                 (mod-t correction of the dropped prime, division)
  fused(...)     the derivation of include/troyn.h: both corrections added in coefficient form, ONE forward transform per output limb
The key-switch inner product is common ground (the fused entry runs the key switch's own steps for it) and is shared.
"""
import random

N = 8


def _is_prime(v):
    return v > 1 and all(v % d for d in range(2, int(v ** 0.5) + 1))


def ntt_primes(count, bits=20, n=N):
    """the `count` largest `bits`-bit primes = 1 mod 2n"""
    out, v = [], (1 << bits) - 1
    v -= (v - 1) % (2 * n)
    while len(out) < count:
        if _is_prime(v):
            out.append(v)
        v -= 2 * n
    return out


def _psi(q, n=N):
    """a primitive 2n-th root of unity mod q"""
    for g in range(2, q):
        r = pow(g, (q - 1) // (2 * n), q)
        if pow(r, n, q) == q - 1:
            return r
    raise ValueError(q)


def ntt(x, q):
    """negacyclic transform: evaluation at the odd powers of psi (any fixed linear bijection with a pointwise product serves the algebra)"""
    psi = _psi(q)
    return [sum(x[k] * pow(psi, (2 * i + 1) * k, q) for k in range(N)) % q for i in range(N)]


def intt(y, q):
    psi = _psi(q)
    ninv = pow(N, -1, q)
    return [ninv * sum(y[i] * pow(psi, -(2 * i + 1) * k, q) for i in range(N)) % q for k in range(N)]


def mul(a, b, q):
    return [x * y % q for x, y in zip(a, b)]


def add(a, b, q):
    return [(x + y) % q for x, y in zip(a, b)]


def sub(a, b, q):
    return [(x - y) % q for x, y in zip(a, b)]


def scale(a, w, q):
    return [x * w % q for x in a]


def inner_product(c2, keys, q, L):
    """P[comp][row], rows 0 .. L-1 and the special row L (modulus q[-1]): SUM_i NTT_row([INTT_i(c2_i)]_{q_row}) . key[i][comp][row];
    keys[i][comp][row] over the K = len(q) key moduli, the special prime last"""
    K = len(q)
    digits = [intt(c2[i], q[i]) for i in range(L)]
    P = [[None] * (L + 1) for _ in range(2)]
    for r in range(L + 1):
        kr = r if r < L else K - 1
        m = q[kr]
        for comp in range(2):
            acc = [0] * N
            for i in range(L):
                acc = add(acc, mul(ntt([d % m for d in digits[i]], m), keys[i][comp][kr], m), m)
            P[comp][r] = acc
    return P


def delta(c, big, inv_big_mod_t, t, qj):
    """bgv_delta_kernel: k = -(c mod t) big^-1 mod t;  [k]_{q_j} big + [c]_{q_j}"""
    out = []
    for v in c:
        k = (-(v % t)) % t * inv_big_mod_t % t
        out.append(((k % qj) * big + v % qj) % qj)
    return out


# ---- the three steps, composed ----
def dyadic_convolute(a, b, q, L):
    return [[mul(a[0][j], b[0][j], q[j]) for j in range(L)],
            [add(mul(a[0][j], b[1][j], q[j]), mul(a[1][j], b[0][j], q[j]), q[j]) for j in range(L)],
            [mul(a[1][j], b[1][j], q[j]) for j in range(L)]]


def bgv_relinearize(c, keys, q, L, t):
    qk = q[-1]
    P = inner_product(c[2], keys, q, L)
    out = []
    for comp in range(2):
        s = intt(P[comp][L], qk)
        rows = []
        for j in range(L):
            d = ntt(delta(s, qk, pow(qk, -1, t), t, q[j]), q[j])
            rows.append(add(scale(sub(P[comp][j], d, q[j]), pow(qk, -1, q[j]), q[j]), c[comp][j], q[j]))
        out.append(rows)
    return out


def bgv_mod_switch(r, q, L, t):
    ql = q[L - 1]
    out = []
    for comp in range(2):
        last = intt(r[comp][L - 1], ql)
        rows = []
        for j in range(L - 1):
            d = ntt(delta(last, ql, pow(ql, -1, t), t, q[j]), q[j])
            rows.append(scale(sub(r[comp][j], d, q[j]), pow(ql, -1, q[j]), q[j]))
        out.append(rows)
    return out


def composed(a, b, keys, q, L, t):
    return bgv_mod_switch(bgv_relinearize(dyadic_convolute(a, b, q, L), keys, q, L, t), q, L, t)


# ---- the fused derivation ----
def fused(a, b, keys, q, L, t, drop_key_correction=False):
    """out_j = (Q_j - NTT_j(dk_j(s) qk^-1 + dl_j(l))) ql^-1;  drop_key_correction: the mutation the GPU tests must catch"""
    qk, ql = q[-1], q[L - 1]
    inv_k_t, inv_l_t = pow(qk, -1, t), pow(ql, -1, t)
    c2 = [mul(a[1][j], b[1][j], q[j]) for j in range(L)]
    P = inner_product(c2, keys, q, L)
    out = []
    for comp in range(2):
        def c(j):
            if comp == 0:
                return mul(a[0][j], b[0][j], q[j])
            return add(mul(a[0][j], b[1][j], q[j]), mul(a[1][j], b[0][j], q[j]), q[j])

        def Q(j):
            return add(scale(P[comp][j], pow(qk, -1, q[j]), q[j]), c(j), q[j])

        s = intt(P[comp][L], qk)
        dk_last = scale(delta(s, qk, inv_k_t, t, ql), pow(qk, -1, ql), ql)
        l = sub(intt(Q(L - 1), ql), dk_last, ql)
        rows = []
        for j in range(L - 1):
            d = delta(l, ql, inv_l_t, t, q[j])
            if not drop_key_correction:
                d = add(scale(delta(s, qk, inv_k_t, t, q[j]), pow(qk, -1, q[j]), q[j]), d, q[j])
            rows.append(scale(sub(Q(j), ntt(d, q[j]), q[j]), pow(ql, -1, q[j]), q[j]))
        out.append(rows)
    return out


def random_case(seed, q, L):
    rng = random.Random(seed)
    K = len(q)
    ct = lambda: [[[rng.randrange(q[j]) for _ in range(N)] for j in range(L)] for _ in range(2)]
    keys = [[[[rng.randrange(q[r]) for _ in range(N)] for r in range(K)] for _ in range(2)] for _ in range(L)]
    return ct(), ct(), keys


def constant_ct(q, L, value):
    """value(q_j) in every word"""
    return [[[value(q[j])] * N for j in range(L)] for _ in range(2)]
