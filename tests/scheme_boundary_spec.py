"""The kernels at the scheme boundary on Python integers: plaintext -> residues (BFV scale-up, centralize), phase -> plaintext (BFV
decrypt_scale_and_round, BGV decrypt_mod_t) and the divisions by the last prime (BFV divide_and_round_q_last, BGV mod_t_and_divide_q_last,
mod_switch_drop).  Nothing here imports the oracle or the package.

Contracts BY DEFINITION (one formula on integers, no algorithm):  bfv_scale_up, plain_centralize, divide_and_round_q_last, mod_switch_drop,
bgv_mod_t_and_divide_q_last, true_round.
RESTATED ALGORITHMS (the result is defined by the steps, not by a closed formula):  bfv_decrypt_scale_and_round (the gamma correction of BEHZ
decryption: away from a rounding boundary it equals true_round, next to one it may not) and bgv_decrypt_mod_t (the quotient of the exact base
conversion is estimated in IEEE doubles, summed in limb order; Python floats are IEEE doubles).

Layouts: one polynomial is uint64 [L][n] (limb-major, as the library stores it); q is the list of the L primes of the level; Q = prod(q).
The input builders at the end are pure functions of (q, t, seed); both test files take their inputs from them.
"""
import math
import random

import numpy as np


# ---- small number theory -------------------------------------------------------------------------------------------------------------

def product(q):
    Q = 1
    for v in q:
        Q *= int(v)
    return Q


def is_prime(n):
    """deterministic Miller-Rabin for n < 2^64"""
    if n < 2:
        return False
    for p in (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37):
        if n % p == 0:
            return n == p
    d, r = n - 1, 0
    while d % 2 == 0:
        d //= 2
        r += 1
    for a in (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37):
        x = pow(a, d, n)
        if x in (1, n - 1):
            continue
        for _ in range(r - 1):
            x = x * x % n
            if x == n - 1:
                break
        else:
            return False
    return True


def prev_prime(bound):
    """the largest prime below bound"""
    v = bound - 1
    while not is_prime(v):
        v -= 1
    return v


def _big(x):
    return np.asarray(x, dtype=np.uint64).astype(object)


def residue_rows(values, q):
    """integers (any sign) -> uint64 [L][len(values)], row j = values mod q_j"""
    vals = np.array([int(v) for v in values], dtype=object)
    return np.stack([(vals % int(qj)).astype(np.uint64) for qj in q])


def crt(x, q):
    """uint64 [L][n] canonical residues -> object [n], the integers in [0, Q)"""
    Q = product(q)
    acc = np.zeros(np.asarray(x).shape[-1], dtype=object)
    for j, qj in enumerate(q):
        qj = int(qj)
        p = Q // qj
        acc = acc + _big(x[j]) * (p * pow(p % qj, -1, qj) if len(q) > 1 else 1)
    return acc % Q


# ---- plaintext -> residues --------------------------------------------------------------------------------------------------------------

def bfv_scale_up(m, q, t, n=None, src=None, subtract=False):
    """scaling_variant::scale_up.  m: plain_coeff_count coefficients in [0, t);  returns uint64 [L][n] (n >= len(m), default len(m)):

        coefficient i < len(m):   dest_j = (src_j or 0) +/- floor((m Q + floor((t+1)/2)) / t)   mod q_j
        coefficient i >= len(m):  dest_j = src_j or 0

    The reference (and the kernel) computes  m floor(Q/t) + floor((m (Q mod t) + (t+1)/2) / t)  per limb.  That is the same integer: write
    Q = t floor(Q/t) + (Q mod t); then m Q + h = t (m floor(Q/t)) + (m (Q mod t) + h), the first term is a multiple of t, and for integers
    a, b:  floor((t a + b) / t) = a + floor(b / t).  (h = floor((t+1)/2) is what the reference calls plain_upper_half_threshold.)"""
    m = _big(m)
    count = m.shape[0]
    n = count if n is None else n
    Q, t = product(q), int(t)
    scaled = (m * Q + (t + 1) // 2) // t
    out = np.zeros((len(q), n), dtype=np.uint64)
    for j, qj in enumerate(q):
        qj = int(qj)
        base = _big(src[j]) if src is not None else np.zeros(n, dtype=object)
        row = base.copy()
        row[:count] = (base[:count] - scaled) % qj if subtract else (base[:count] + scaled) % qj
        out[j] = row.astype(np.uint64)
    return out


def plain_centralize(m, q, t, n=None):
    """scaling_variant::centralize: the plaintext coefficient as a centred integer in (-t/2, t/2], reduced by every q_l:

        m >= floor((t+1)/2) ?  (m + Q - t) mod q_l  :  m mod q_l           zero beyond len(m)

    Q = 0 mod q_l, so this is (m - t) mod q_l: valid for t below q_l (the reference's fast plain lift: m + (q_l - t), no reduction needed),
    above q_l, and a multiple of q_l (the increment is then 0 mod q_l)."""
    m = _big(m)
    count = m.shape[0]
    n = count if n is None else n
    Q, t = product(q), int(t)
    lifted = np.array([v + Q - t if v >= (t + 1) // 2 else v for v in m], dtype=object)
    out = np.zeros((len(q), n), dtype=np.uint64)
    for l, ql in enumerate(q):
        out[l, :count] = (lifted % int(ql)).astype(np.uint64)
    return out


# ---- divisions by the last prime ----------------------------------------------------------------------------------------------------------

def divide_and_round_q_last(x, q):
    """RNSTool::divide_and_round_q_last (BFV, coefficient form).  x uint64 [L][n] canonical -> uint64 [L-1][n].  With X the CRT integer of x:

        r = ((X mod q_last) + h) mod q_last - h,   h = q_last >> 1        (the centred remainder: -h <= r <= q_last - 1 - h)
        out_j = (X - r) / q_last  mod q_j                                  (an exact division)"""
    L = len(q)
    ql = int(q[L - 1])
    h = ql >> 1
    X = crt(x, q)
    r = (X % ql + h) % ql - h
    assert all(int(v) % ql == 0 for v in (X - r)[:4])
    quo = (X - r) // ql
    return np.stack([(quo % int(q[j])).astype(np.uint64) for j in range(L - 1)])


def mod_switch_drop(x, L_out):
    """Evaluator::mod_switch_drop_to: the first L_out limbs, nothing else"""
    return np.ascontiguousarray(np.asarray(x, dtype=np.uint64)[:L_out])


def bgv_mod_t_and_divide_q_last(x, q, t):
    """RNSTool::mod_t_and_divide_q_last (BGV), in coefficient form.  x uint64 [L][n] canonical -> uint64 [L-1][n]:

        k = -(c_last mod t) q_last^-1  mod t          (c_last = the last row; q_last must be invertible mod t)
        delta = k q_last + c_last                     (= 0 mod t and = c_last mod q_last: what is subtracted changes nothing modulo t)
        out_j = (c_j - delta) q_last^-1  mod q_j"""
    L, t = len(q), int(t)
    ql = int(q[L - 1])
    inv_t = pow(ql % t, -1, t)
    c_last = _big(x[L - 1])
    k = (-(c_last % t) * inv_t) % t
    delta = k * ql + c_last
    assert all(int(d) % t == 0 for d in delta[:4])
    return np.stack([(((_big(x[j]) - delta) * pow(ql % int(q[j]), -1, int(q[j]))) % int(q[j])).astype(np.uint64) for j in range(L - 1)])


# ---- phase -> plaintext -------------------------------------------------------------------------------------------------------------------

def _inv_punctured(q):
    """(Q/q_i)^-1 mod q_i; 1 for a base of one prime (the empty product)"""
    Q = product(q)
    return [pow((Q // int(qi)) % int(qi), -1, int(qi)) if len(q) > 1 else 1 for qi in q]


def bgv_double_sum(y, q):
    """the quotient estimate of BaseConverter::exact_convey_array: SUM_i double(y_i) / double(q_i), summed in limb order from 0.0"""
    v = 0.0
    for yi, qi in zip(y, q):
        v += float(int(yi)) / float(int(qi))
    return v


def round_half_away(v):
    """std::round for v >= 0 without forming v + 0.5 (which would round a second time): the fraction v - floor(v) is exact in doubles"""
    r = math.floor(v)
    return r + 1 if v - r >= 0.5 else r


def bgv_fast_conversion_terms(column, q):
    """y_i = x_i (Q/q_i)^-1 mod q_i of one coefficient (x_i any 64-bit word)"""
    return [int(x) % int(qi) * ip % int(qi) for x, qi, ip in zip(column, q, _inv_punctured(q))]


def bgv_decrypt_mod_t(phase, q, t, correction=1):
    """RNSTool::decrypt_mod_t = exact_convey_array q -> {t}, then times correction^-1 mod t (scaling_variant::decentralize).
    phase uint64 [L][n] -> list of n integers in [0, t).  A RESTATED ALGORITHM: y_i on integers, v = round(SUM_i double(y_i)/double(q_i)) in
    doubles (limb order, halves away from zero), out = (SUM_i y_i (Q/q_i mod t) - v (Q mod t)) correction^-1 mod t on integers."""
    t = int(t)
    Q = product(q)
    ip = _inv_punctured(q)
    punct_t = [(Q // int(qi)) % t for qi in q]
    fix = pow(int(correction) % t, -1, t)
    out = []
    for c in range(np.asarray(phase).shape[-1]):
        y = [int(phase[i][c]) % int(qi) * ip[i] % int(qi) for i, qi in enumerate(q)]
        v = round_half_away(bgv_double_sum(y, q))
        out.append((sum(yi * p for yi, p in zip(y, punct_t)) - v * (Q % t)) * fix % t)
    return out


def bfv_decrypt_scale_and_round(phase, q, t, gamma):
    """RNSTool::decrypt_scale_and_round (BEHZ decryption), A RESTATED ALGORITHM.  phase uint64 [L][n] -> list of n integers in [0, t):

        y_i = x_i (gamma t mod q_i) (Q/q_i)^-1  mod q_i
        s_t = -Q^-1 SUM_i y_i (Q/q_i)  mod t          s_g = the same mod gamma       (fast base conversion of gamma t x to {t, gamma}, divided by -Q)
        out = (s_t - centred(s_g)) gamma^-1  mod t,   centred(s) = s - gamma if s > gamma >> 1 else s"""
    t, gamma = int(t), int(gamma)
    Q = product(q)
    ip = _inv_punctured(q)
    punct = [Q // int(qi) for qi in q]
    neg_inv_t, neg_inv_g = (-pow(Q % t, -1, t)) % t, (-pow(Q % gamma, -1, gamma)) % gamma
    inv_gamma = pow(gamma % t, -1, t)
    out = []
    for c in range(np.asarray(phase).shape[-1]):
        y = [int(phase[i][c]) % int(qi) * (gamma * t % int(qi)) % int(qi) * ip[i] % int(qi) for i, qi in enumerate(q)]
        total = sum(yi * p for yi, p in zip(y, punct))
        s_t, s_g = total % t * neg_inv_t % t, total % gamma * neg_inv_g % gamma
        d = (s_t + (gamma - s_g) % t) % t if s_g > gamma >> 1 else (s_t - s_g % t) % t
        out.append(d * inv_gamma % t)
    return out


def true_round(x, Q, t):
    """round(t x / Q) mod t with halves up: what decryption means"""
    return (2 * int(t) * int(x) + int(Q)) // (2 * int(Q)) % int(t)


# ---- input builders: pure functions of (q, t, seed) -----------------------------------------------------------------------------------------

def unique(values):
    seen, out = set(), []
    for v in values:
        if v not in seen:
            seen.add(v)
            out.append(v)
    return out


def scale_up_edges(q, t, seed):
    """plaintext coefficients where bfv_scale_up can go wrong: the ends of [0, t), either side of the sign threshold, the m at which the inner
    quotient floor((m r + h) / t) steps (r = Q mod t, h = (t+1)//2: (m r + h) mod t in {0, 1, t-1}; they exist when gcd(r, t) = 1), and the
    m that make m r largest (t-1, t-2 and seeded values in the top sixteenth of [0, t)): at a wide t their product does not fit one word."""
    t = int(t)
    r, h = product(q) % t, (t + 1) // 2
    vals = [0, 1, t - 1, (t - 1) // 2, (t + 1) // 2]
    if math.gcd(r, t) == 1:
        inv = pow(r, -1, t)
        vals += [(target - h) * inv % t for target in (0, 1, t - 1)]
    vals += [t - 1, max(t - 2, 0)]
    rng = random.Random(seed)
    vals += [t - 1 - rng.randrange(t // 16 + 1) for _ in range(6)]
    return unique(v % t for v in vals)


def round_boundary_ks(t, seed):
    rng = random.Random(seed)
    return [rng.randrange(int(t)) for _ in range(32)]


def round_boundaries(q, t, seed):
    """phases (integers in [0, Q)) either side of t x / Q = k + 1/2 for the 32 k of round_boundary_ks: x = ceil((2k+1) Q / (2t)) and x - 1, in
    that order; then 0, 1, Q-1, Q//2, Q//2+1.  (For Q >= t: true_round(x) = k + 1 mod t and true_round(x - 1) = k.)"""
    Q, t = product(q), int(t)
    out = []
    for k in round_boundary_ks(t, seed):
        x = -((-(2 * k + 1) * Q) // (2 * t))
        out += [x % Q, (x - 1) % Q]
    return out + [0, 1 % Q, Q - 1, Q // 2, (Q // 2 + 1) % Q]


def half_integer_phases(q, seed, count=64):
    """raw phase words uint64 [L][count] (L = 2 or 3) whose exact SUM_i y_i / q_i is k + 1/2 + d / (2Q) with a small odd d: the double sum that
    bgv_decrypt_mod_t rounds lies within an ulp or two of a half-integer, so the result depends on every rounding of the divisions and of the sum.

    y -> SUM_i y_i (Q/q_i) is a bijection from PROD [0, q_i) onto the classes mod Q, so SUM_i y_i (Q/q_i) = (Q + d)/2 + k Q has exactly one
    solution y per odd d (k in [0, L) is whatever that y gives).  Coefficients 0 and 1 take d = +1 and -1; as two coefficients are not a test, the
    others take seeded odd d with |d| < 2^20: still d / (2Q) < 2^-59 for Q > 2^79, a thousandth of an ulp of 0.5.  The raw word of limb i is
    T mod q_i for T = (Q + d)/2: the kernel's own multiplication by (Q/q_i)^-1 then yields y_i."""
    assert len(q) in (2, 3)
    Q = product(q)
    rng = random.Random(seed)
    ds = [1, -1] + [(2 * rng.randrange(1 << 19) + 1) * rng.choice((1, -1)) for _ in range(count - 2)]
    return residue_rows([(Q + d) // 2 for d in ds], q)


def bgv_last_limb_edges(q, t, seed):
    """coefficient columns uint64 [L][count] for the BGV division by q_last.  The last row takes 0, 1, q_last - 1 and values with
    c_last mod t in {0, 1, t-1} (the largest such value below q_last and a seeded one); the other rows of those columns cycle through the corner
    values q_j - 1, 0, q_j - 1, 1 (alternating).  The last two columns are the residues of the centred +floor(Q/2) and -floor(Q/2)."""
    L, t = len(q), int(t)
    ql = int(q[L - 1])
    rng = random.Random(seed)
    last = [0, 1, ql - 1]
    for rem in (0, 1, t - 1):
        if rem >= ql:
            continue
        top = (ql - 1 - rem) // t
        last += [top * t + rem, rng.randrange(top + 1) * t + rem]
    last = unique(last)
    cols = np.zeros((L, len(last)), dtype=np.uint64)
    cols[L - 1] = np.array(last, dtype=np.uint64)
    for j in range(L - 1):
        corner = [int(q[j]) - 1, 0, int(q[j]) - 1, 1]
        cols[j] = np.array([corner[(c + j) % 4] for c in range(len(last))], dtype=np.uint64)
    Q = product(q)
    return np.concatenate([cols, residue_rows([Q // 2, -(Q // 2)], q)], axis=1)


def tile_columns(cols, n, filler):
    """[L][count] edge columns at the front of [L][n]; the rest comes from filler (uint64 [L][n], e.g. uniform residues)"""
    out = np.array(filler, dtype=np.uint64, copy=True)
    count = min(cols.shape[1], n)
    out[:, :count] = cols[:, :count]
    return out


# ---- the parameter sets both test files run (chains as bit sizes: the tests turn them into primes = 1 mod 2N) ------------------------------

SEED = 2
SCALE_UP_CHAINS = ([60, 60, 60], [50, 50], [36, 36, 37], [30, 30, 30])
CENTRALIZE_CHAINS = ([30, 30, 30], [60, 40, 40, 60])
BGV_CHAINS = ([30, 30, 30], [36, 36, 37], [60, 40, 40, 60])
DECRYPT_MOD_T_CHAINS = ([40, 40, 40], [60, 60, 60])
DIVIDE_CHAINS = ([50, 50, 50, 50], [60, 40, 40, 60], [36, 36, 37])


def scale_up_plain_moduli():
    """2^40 - 87 is the largest prime below 2^40; the last entry, and every entry against the 30-bit chain, is above the primes of the chain;
    from 2^40 - 87 on, (t - 1) (Q mod t) needs the high word of the 128-bit quotient (test_scheme_boundary_spec.py asserts it)"""
    return [2, 3, 65537, 1 << 20, (1 << 40) - 87, 1 << 59, prev_prime(1 << 59), prev_prime(1 << 61)]


def centralize_plain_moduli(bits, q):
    """30-bit chain: a 40-bit prime (above every q_l), 2 q_0 (a multiple of q_0), q_1 itself, 2^45; {60,40,40,60}: 2, 2^21 (below every q_l) and
    2^59 (between the 40-bit and the 60-bit limbs)"""
    if list(bits) == [30, 30, 30]:
        return [prev_prime(1 << 40), 2 * int(q[0]), int(q[1]), 1 << 45]
    return [2, 1 << 21, 1 << 59]


def bgv_plain_moduli(n):
    """t = 2N: every q_i = 1 mod 2N, so q_last^-1 mod t = 1 and bgv_delta_kernel skips its multiplication; the 49-bit prime is above the 30-,
    36- and 40-bit limbs (k is reduced by q_j before it is multiplied)"""
    return [2, 2 * n, 257, 65537, 1 << 20, prev_prime(1 << 49)]


def decrypt_mod_t_plain_moduli():
    return [65537, 1 << 20, prev_prime(1 << 49), 1 << 59]


def scale_up_inputs(q, t, seed, uniform):
    """scale_up_edges at the front of the uniform coefficients the caller drew"""
    edges = scale_up_edges(q, t, seed)
    m = [int(v) for v in uniform]
    m[:len(edges)] = edges[:len(m)]
    return m


def noisy_scale_ups(m, q, t):
    """x = scale_up(m) + e mod Q, e cycling through both ends of [-Q//(4t), Q//(4t)], their inner neighbours, -1, 0 and 1 (shifted by one every
    seven coefficients, so that the edges at the front of m meet different e)"""
    Q, t = product(q), int(t)
    bound = Q // (4 * t)
    noise = [-bound, bound, -bound + 1, bound - 1, -1, 0, 1]
    return [((int(v) * Q + (t + 1) // 2) // t + noise[(i + i // len(noise)) % len(noise)]) % Q for i, v in enumerate(m)]


def divide_edges(q):
    """integers in [0, Q) for the divisions by q_last: 0, 1, Q-1, the centred +-floor(Q/2), and X with X mod q_last in {h-1, h, h+1} (h = q_last >> 1:
    either side of where the centred remainder changes sign) on top of small, middle and large multiples of q_last"""
    Q = product(q)
    ql = int(q[-1])
    h = ql >> 1
    out = [0, 1 % Q, Q - 1, Q // 2, (-(Q // 2)) % Q]
    for base in (0, (Q // ql // 2) * ql, Q - ql):
        out += [(base + r) % Q for r in (h - 1, h, h + 1)]
    return out
