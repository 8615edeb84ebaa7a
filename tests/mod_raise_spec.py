"""CKKS ModRaise (troyn_ckks_mod_raise, include/troyn.h) restated on Python integers.

The contract: per coefficient position (coefficient form), x = the centred representative in (-Q/2, Q/2] of the L_in input residues,
Q = q_0 ... q_{L_in-1} (X > floor(Q/2) stands for X - Q); row j of the result is x mod q_j in [0, q_j) for every j < L_out.

Two forms that must agree word for word:
  mod_raise_rows         the contract itself, on big integers (CRT composition, centring, one % per target prime);
  mod_raise_mixed_radix  what the kernel does without multi-word arithmetic: the mixed-radix (Garner) digits d_i of X, the comparison with
                         floor(Q/2) as a lexicographic comparison of the digits from the top, and per target prime a Horner over the digits
                         r = (r (q_i mod q_j) + d_i) mod q_j, minus Q mod q_j where X was above the half.
"""
import numpy as np


def product(primes):
    q = 1
    for p in primes:
        q *= int(p)
    return q


def compose(residues, primes):
    """X in [0, Q) of every column of residues [L][n] (CRT); a list of Python integers"""
    primes = [int(p) for p in primes]
    Q = product(primes)
    cols = np.asarray(residues).astype(object)
    total = np.zeros(cols.shape[1], dtype=object)
    for i, q in enumerate(primes):
        punctured = Q // q
        total = total + cols[i] * (punctured * pow(punctured % q, -1, q))
    return [int(v) % Q for v in total]


def centre(X, Q):
    """the representative in (-Q/2, Q/2]"""
    return X - Q if X > Q // 2 else X


def residues_of(values, primes):
    """[L][n] uint64 residues of signed integers"""
    return np.array([[int(v) % int(q) for v in values] for q in primes], dtype=np.uint64)


def mod_raise_rows(residues, primes, L_in, L_out):
    """residues [L_in][n] canonical words under primes[:L_in] -> [L_out][n] uint64 under primes[:L_out]"""
    assert 1 <= L_in < L_out <= len(primes) and len(residues) == L_in
    Q = product(primes[:L_in])
    xs = [centre(X, Q) for X in compose(residues, primes[:L_in])]
    return residues_of(xs, primes[:L_out])


# ---- the mixed-radix form -------------------------------------------------------------------------------------------------------------
def mixed_radix_digits(column, primes):
    """d with X = d_0 + q_0 (d_1 + q_1 (d_2 + ...)), 0 <= d_i < q_i (Garner's recurrence on words below the prime)"""
    d = []
    for i, q in enumerate(primes):
        v = int(column[i]) % q
        for j in range(i):
            v = ((v - d[j]) * pow(int(primes[j]) % q, -1, q)) % q
        d.append(v)
    return d


def digits_of_integer(X, primes):
    """the mixed-radix digits of an integer 0 <= X < Q by division"""
    d = []
    for q in primes:
        d.append(X % q)
        X //= q
    assert X == 0
    return d


def integer_of_digits(d, primes):
    X = 0
    for di, q in zip(reversed(d), reversed(primes)):
        X = X * q + di
    return X


def above_half(d, half):
    """X > floor(Q/2), decided at the highest digit that differs"""
    for i in range(len(d) - 1, -1, -1):
        if d[i] != half[i]:
            return d[i] > half[i]
    return False


def mod_raise_mixed_radix(residues, primes, L_in, L_out):
    primes = [int(p) for p in primes]
    assert 1 <= L_in < L_out <= len(primes) and len(residues) == L_in
    inp = primes[:L_in]
    Q = product(inp)
    half = digits_of_integer(Q // 2, inp)
    res = np.asarray(residues, dtype=np.uint64)
    n = res.shape[1]
    out = np.zeros((L_out, n), dtype=np.uint64)
    out[:L_in] = res
    for x in range(n):
        d = mixed_radix_digits([int(v) for v in res[:, x]], inp)
        greater = above_half(d, half)
        for j in range(L_in, L_out):
            qj = primes[j]
            r = 0
            for i in range(L_in - 1, -1, -1):
                r = (r * (inp[i] % qj) + d[i]) % qj
            if greater:
                r = (r - Q % qj) % qj
            out[j, x] = r
    return out


# ---- the values every test plants --------------------------------------------------------------------------------------------------------
def planted_values(primes_in):
    """signed integers around every boundary of the centring: 0, 1, -1, floor(Q/2), floor(Q/2) + 1 (= -(Q - floor(Q/2) - 1)), Q - 1 (= -1),
    floor(Q/2) +- q_0"""
    Q = product(primes_in)
    h, q0 = Q // 2, int(primes_in[0])
    return [0, 1, -1, h, h + 1, Q - 1, h + q0, h - q0]


def tie_values(primes_in, rng):
    """X whose digits above position k equal those of floor(Q/2) and whose digit k is one off (both sides), random below: the comparison is decided
    at digit k, for every k"""
    primes_in = [int(p) for p in primes_in]
    half = digits_of_integer(product(primes_in) // 2, primes_in)
    out = []
    for k in range(len(primes_in)):
        for step in (-1, 1):
            dk = half[k] + step
            if 0 <= dk < primes_in[k]:
                d = [int(rng.integers(0, q)) for q in primes_in[:k]] + [dk] + half[k + 1:]
                out.append(integer_of_digits(d, primes_in))
        # ... and equal at digit k too, decided below or not at all
        out.append(integer_of_digits([0] * k + half[k:], primes_in))
    return out
