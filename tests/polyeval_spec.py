"""The fixed schedule of Evaluator::evaluate_polynomial (troy/troy.h) restated in Python, and a noise-free simulation of it on exact
rationals: a ciphertext is (value, scale, limbs) with value = round(message * scale) an integer, a rescale is the exact division by the
last prime with rounding."""
from fractions import Fraction


def clog2(v):
    r = 0
    while (1 << r) < v:
        r += 1
    return r


def degree(coefficients):
    d = len(coefficients)
    while d and coefficients[d - 1] == 0:
        d -= 1
    if d == 0:
        raise ValueError("all coefficients are zero")
    return d - 1


def schedule(d):
    """(k, g, needed powers, total depth)"""
    if d <= 1:
        return 1, 1, set(), 1
    k = 2
    while k * k < d + 1:
        k *= 2
    g = -(-(d + 1) // k)
    needed = set(range(2, k)) | {k} | {j * k for j in range(1, g)}
    return k, g, needed, max(clog2((g - 1) * k), clog2(k) + 1) + 1


def split(m):
    """x^m = x^a * x^(m - a): a power of two is the square of x^(m/2), any other m takes the largest power of two below m"""
    a = 1
    while a * 2 < m:
        a *= 2
    return a, m - a


def power_depth(m):
    return clog2(m)


def _round(fr):
    return (2 * fr.numerator + fr.denominator) // (2 * fr.denominator)      # round half up: exact integers


class Ct:
    def __init__(self, value, scale, limbs):
        self.value, self.scale, self.limbs = value, Fraction(scale), limbs


def simulate(message, coefficients, scale, primes):
    """-> (addends of the final sum as Ct at the result's level, result Ct, multiplications done).  `primes`: the data primes of the chain."""
    d = degree(coefficients)
    k, g, needed, depth = schedule(d)
    L0 = len(primes)
    assert L0 >= depth + 1
    coef = lambda m: Fraction(coefficients[m]) if m <= d else Fraction(0)
    x = Ct(_round(Fraction(message) * scale), scale, L0)
    rescale = lambda c: Ct(_round(Fraction(c.value, primes[c.limbs - 1])), c.scale / primes[c.limbs - 1], c.limbs - 1)
    muls = []

    def leaf(ins, limbs, sum_scale, cs):
        assert all(c.limbs >= limbs for c in ins)      # taller inputs are cut, never raised
        v = _round(cs[0] * sum_scale)
        for c, w in zip(ins, cs[1:]):
            v += _round(w * (sum_scale / c.scale)) * c.value
        return rescale(Ct(v, sum_scale, limbs))

    if d <= 1:
        out = leaf([x], L0, Fraction(scale) * primes[L0 - 1], [coef(0), coef(1)])
        return [out], out, muls
    memo = {1: x}

    def power(m):
        if m not in memo:
            a, b = split(m)
            pa, pb = power(a), power(b)
            limbs = min(pa.limbs, pb.limbs)
            memo[m] = rescale(Ct(pa.value * pb.value, pa.scale * pb.scale, limbs))
            muls.append(m)
            assert memo[m].limbs == L0 - power_depth(m)
        return memo[m]

    babies = [power(i) for i in range(1, k)]
    rec = max(clog2((g - 1) * k), clog2(k) + 1)
    Lrec = L0 - rec
    giants = [power(j * k) for j in range(1, g)]
    assert all(G.limbs >= Lrec for G in giants)
    T = Fraction(scale) * primes[Lrec - 1]
    addends = []
    for j in range(1, g):
        lf = leaf(babies, Lrec + 1, T / giants[j - 1].scale * primes[Lrec], [coef(j * k + i) for i in range(k)])
        addends.append(Ct(lf.value * giants[j - 1].value, lf.scale * giants[j - 1].scale, Lrec))
    total = Ct(sum(a.value for a in addends), addends[0].scale, Lrec)
    out = rescale(total)
    leaf0 = leaf(babies, Lrec, T, [coef(i) for i in range(k)])
    final = [rescale(a) for a in addends] + [leaf0]
    assert set(memo) - {1} == needed
    return final, Ct(out.value + leaf0.value, out.scale, out.limbs), muls
