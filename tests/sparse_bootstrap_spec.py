"""Specification of the sparsely packed CKKS bootstrap (troy/bootstrap.h "Sparse packing"; include/troyn.h "Factors of the special DFT on n slots"),
in Python integers and float64.  No GPU.

N is the ring degree, n a power of two with 2 <= n <= N/2, s = N/(2n), Y = X^s, zeta = exp(2 pi i / 2N).  A sparsely packed message is p(Y) of degree
< 2n with coefficients t'; w_k = t'_k + i t'_{k+n}; slot j of the full ring evaluates p at zeta^(s 3^j), and the N/2 slots are an n-vector repeated s times.

table         the factors of the sub-ring's special DFT, zh = L_{m'-1} ... L_0 BR w with m' = log2 n: layer b's twiddle is the full ring's layer b, so
              the table is tests/dft_factors_spec.py's table taken on n rows of the FULL ring's tables -- diagonal indices mod n, first + count <= m',
              the wrap where first + count == m'.  Same association, same roundings.  With n = N/2 it is dft_factors_spec.table.
automorphism  t(X) -> t(X^g) mod X^N + 1 on exact integers; the rotation by r slots is g = 3^r mod 2N.
sub_sum       SUM_{i < s} sigma_{3^(n i)}(t), which is s times the Y-part of t; sub_sum_stages the stages of Evaluator::sub_sum (radix 0: 4), and
              sub_sum_staged the product PROD_i (1 + rot_{n 2^i}) evaluated stage by stage.
pipeline      t = D p(Y) + q0 I(X) with dense I -> p, the chain of Evaluator::bootstrap for a sparse plan in float64: the Y-part times s, the relabel to
              q0, CoeffToSlot on n slots with c1 / s, split, EvalMod, join, SlotToCoeff on n slots with c2, the scale set to D.
"""
import numpy as np

import bootstrap_spec as B
import ckks_encode_spec as E
import dft_factors_spec as D

MASK_NONE, MASK_EVEN, MASK_ODD = D.MASK_NONE, D.MASK_EVEN, D.MASK_ODD
DEFAULT_RADIX = 4


def check_n(big_n, n):
    m = D.log2_exact(n)
    assert 2 <= n <= big_n // 2
    return m


def diagonal_indices(n, first, count):
    return D.diagonal_indices(n, first, count)


def diagonal_count(n, first, count):
    return len(D.diagonal_indices(n, first, count))


def table(tables, n, first, count, inverse=False, col_mask=MASK_NONE, row_mask=MASK_NONE, conjugate=False, constant=1.0):
    """float64 [nd][n][2]: dft_factors_spec.table on n rows; the twiddles are the full ring's (tables = the handle's own, root_powers of N entries)"""
    roots = np.asarray(tables[1], dtype=np.float64)
    log_n = D.log2_exact(len(roots))
    check_n(len(roots), n)
    ds = np.array(D.diagonal_indices(n, first, count), dtype=np.int64)
    row = np.broadcast_to(np.arange(n, dtype=np.int64)[None, :], (len(ds), n))
    col = (row + ds[:, None]) & (n - 1)
    bits = ((1 << count) - 1) << first
    present = ((row ^ col) & ~bits) == 0
    for mask, index in ((row_mask, row), (col_mask, col)):
        if mask != MASK_NONE:
            present = present & ((index & 1) == (1 if mask == MASK_ODD else 0))
    ar, ai = np.full(row.shape, np.float64(constant)), np.zeros(row.shape)
    half = np.float64(0.5)
    order = range(first + count - 1, first - 1, -1) if inverse else range(first, first + count)
    for b in order:
        rb, cb = ((row >> b) & 1) == 1, ((col >> b) & 1) == 1
        lh = 1 << b
        tr, ti = D._twiddles(roots, log_n, b, (col if inverse else row) & (lh - 1))
        if inverse:
            ti = -ti
        neg = cb if inverse else rb
        tr, ti = np.where(neg, -tr, tr), np.where(neg, -ti, ti)
        pr, pi = D._mul(ar, ai, tr, ti)
        use = rb if inverse else cb
        ar, ai = np.where(use, pr, ar), np.where(use, pi, ai)
        if inverse:
            ar, ai = ar * half, ai * half
    if conjugate:
        ai = -ai
    out = np.zeros((len(ds), n, 2), dtype=np.float64)
    out[..., 0], out[..., 1] = np.where(present, ar, 0.0), np.where(present, ai, 0.0)
    return out


def apply(tab, n, first, count, x_re, x_im):
    return D.apply(tab, n, first, count, x_re, x_im)


def direct_slots(t_sub, big_n):
    """p(Y) at zeta^(s 3^j), j < n, from exact integer exponents: t_sub the 2n coefficients of p -> (re [n], im [n])"""
    n = len(t_sub) // 2
    s = big_n // (2 * n)
    t_sub = np.asarray(t_sub, dtype=np.float64)
    re, im = np.zeros(n), np.zeros(n)
    g = 1
    for j in range(n):
        e = np.array([(s * g * k) % (2 * big_n) for k in range(2 * n)], dtype=np.float64)
        angle = e * (np.pi / big_n)
        re[j], im[j] = float(np.sum(t_sub * np.cos(angle))), float(np.sum(t_sub * np.sin(angle)))
        g = g * 3 % (2 * big_n)
    return re, im


# ---- SubSum on exact integers ---------------------------------------------------------------------------------------------------------------

def automorphism(t, g):
    """t(X^g) mod X^N + 1, g odd: a list of Python integers"""
    big_n = len(t)
    out = [0] * big_n
    for k, v in enumerate(t):
        e = k * g % (2 * big_n)
        if e >= big_n:
            out[e - big_n] -= v
        else:
            out[e] += v
    return out


def rotate(t, steps):
    return automorphism(t, pow(3, steps, 2 * len(t)))


def _add(a, b):
    return [x + y for x, y in zip(a, b)]


def y_part(t, n):
    """the part of t that is a polynomial in Y = X^s"""
    s = len(t) // (2 * n)
    return [v if k % s == 0 else 0 for k, v in enumerate(t)]


def sub_sum(t, n):
    s = len(t) // (2 * n)
    out = [0] * len(t)
    for i in range(s):
        out = _add(out, rotate(t, n * i))
    return out


def sub_sum_stages(slot_count, n, radix=0):
    """Evaluator::sub_sum_stages: the non-zero steps of every stage, in order"""
    D.log2_exact(slot_count)
    D.log2_exact(n)
    assert 2 <= n <= slot_count
    radix = DEFAULT_RADIX if radix == 0 else radix
    assert radix >= 2 and D.log2_exact(radix) >= 1
    stages, step = [], n
    while step < slot_count:
        terms = min(radix, slot_count // step)
        stages.append([i * step for i in range(1, terms)])
        step *= terms
    return stages


def sub_sum_steps(slot_count, n, radix=0):
    return sorted({x for stage in sub_sum_stages(slot_count, n, radix) for x in stage})


def sub_sum_staged(t, n, radix=0):
    cur = list(t)
    for stage in sub_sum_stages(len(t) // 2, n, radix):
        nxt = list(cur)
        for step in stage:
            nxt = _add(nxt, rotate(cur, step))
        cur = nxt
    return cur


# ---- the float64 chain ----------------------------------------------------------------------------------------------------------------------

def coeff_to_slot(tables, z_re, z_im, groups, constant):
    """bootstrap_spec.coeff_to_slot on the n = len(z) slots of the sub-ring"""
    n = len(z_re)
    m = D.log2_exact(n)
    assert sum(groups) == m
    done, re, im = 0, np.asarray(z_re, dtype=np.float64), np.asarray(z_im, dtype=np.float64)
    for g, (count, c) in enumerate(zip(groups, B._group_constants(constant, len(groups)))):
        done += count
        first = m - done
        if g == 0:
            er, ei = apply(table(tables, n, first, count, inverse=True, col_mask=MASK_EVEN, constant=c), n, first, count, re, im)
            orr, oi = apply(table(tables, n, first, count, inverse=True, col_mask=MASK_ODD, conjugate=True, constant=c), n, first, count, re, im)
            re, im = er + orr, ei - oi
        else:
            re, im = apply(table(tables, n, first, count, inverse=True, constant=c), n, first, count, re, im)
    return re, im


def slot_to_coeff(tables, y_re, y_im, groups, constant):
    n = len(y_re)
    assert sum(groups) == D.log2_exact(n)
    done, re, im = 0, np.asarray(y_re, dtype=np.float64), np.asarray(y_im, dtype=np.float64)
    for g, (count, c) in enumerate(zip(groups, B._group_constants(constant, len(groups)))):
        first = done
        done += count
        if g == len(groups) - 1:
            er, ei = apply(table(tables, n, first, count, row_mask=MASK_EVEN, constant=c), n, first, count, re, im)
            orr, oi = apply(table(tables, n, first, count, row_mask=MASK_ODD, constant=c), n, first, count, re, im)
            re, im = er + orr, ei - oi
        else:
            re, im = apply(table(tables, n, first, count, constant=c), n, first, count, re, im)
    return re, im


def pipeline(t, n, primes, delta, half_width, degree, double_angles, down_groups, up_groups, weight_scale, tables):
    """coefficients t = D p(Y) + q0 I(X) (float64, N of them, I dense) -> the N coefficients of p(Y) (zero off the multiples of s), and the constants"""
    big_n = len(t)
    slot_count = big_n // 2
    s = slot_count // n
    k = B.plan_constants(primes, delta, half_width, degree, double_angles, down_groups, up_groups, weight_scale)
    q0 = float(primes[0])
    t = np.asarray(t, dtype=np.float64)
    u = np.where(np.arange(big_n) % s == 0, t * float(s), 0.0)            # 2b. sub_sum: s times the Y-part
    x = (u / delta) * (delta / q0)                                        # 3. the relabel D -> q0
    z_re, z_im = E.simd_from_coefficients(x, tables)                      # the full ring's slots: an n-vector repeated s times
    tiled = np.max(np.abs(np.tile(z_re[:n], s) - z_re)) + np.max(np.abs(np.tile(z_im[:n], s) - z_im))
    assert tiled <= 1e-9 * (np.max(np.abs(z_re)) + np.max(np.abs(z_im)) + 1.0), tiled
    w_re, w_im = coeff_to_slot(tables, z_re[:n], z_im[:n], down_groups, k["c1"] / float(s))      # 4. c1 BR(x'_k + i x'_{k+n})
    sign = np.where(np.arange(n) % 2 == 0, 1.0, -1.0)
    re2, ims = 2.0 * w_re, sign * 2.0 * w_im                              # 5.
    relabel = k["s1"] / k["part"]
    coeffs = B.interpolant(half_width, degree, double_angles)
    re = B.eval_mod_scheduled(re2 * relabel, half_width, coeffs, double_angles)      # 6.
    im = B.eval_mod_scheduled(ims * relabel, half_width, coeffs, double_angles)
    y_re, y_im = re, sign * im                                            # 7.
    o_re, o_im = slot_to_coeff(tables, y_re, y_im, up_groups, k["c2"])    # 8.
    o_re, o_im = o_re * (k["s2"] / delta), o_im * (k["s2"] / delta)       # 9.
    return E.simd_coefficients(np.tile(o_re, s), np.tile(o_im, s), 1.0, tables), k
