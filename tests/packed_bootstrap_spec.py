"""Specification of the packed sparse CKKS bootstrap (troy/bootstrap.h and troy/slot_transform.h "Packed"; include/troyn.h "Factors of the special DFT on
n slots, both halves on period 2n"), in float64.  No GPU.

N is the ring degree, n a power of two with 2 <= n <= N/4 (the plans: 4 <= n), m' = log2 n.  Layers [first, first + count) with first + count <= m' are
block diagonal with blocks of at most n rows: on 2n rows they are sparse_bootstrap_spec.table(tables, 2n, first, count, ...), two identical n x n blocks,
never the top group there (2^(count+1) - 1 diagonals, indices mod 2n), and no entry crosses row n.

table          float64 [nd][2n][2]: rows < n that table, rows >= n the same words turned by a quarter -- inverse by -i, (re, im) -> (im, -re); forward by +i,
               (re, im) -> (-im, re) -- a swap and one IEEE negation (a zero component of a present entry becomes -0.0); absent entries stay +0.
coeff_to_slot  sparse_bootstrap_spec.coeff_to_slot whose last-applied group (layers [0, c)) is the packed inverse table on the operand tiled to 2n:
               v = M1 u = [G u; -i G u] and P = v + conj(v) = [2 Re(G u); 2 Im(G u)], a real vector of period 2n.
slot_to_coeff  takes the real P' = [a; b]; its first-applied group is the packed forward table, V = F1 P' = [F a; i F b], and V + rot_n(V) = F (a + i b) on
               period n; the remaining groups are sparse_bootstrap_spec's.
pipeline       sparse_bootstrap_spec.pipeline with ONE EvalMod operand: no split, no (-1)^j sign, no join; the same relabel, factor 2 and c1 / s.
"""
import numpy as np

import bootstrap_spec as B
import ckks_encode_spec as E
import dft_factors_spec as D
import sparse_bootstrap_spec as S


def check(big_n, n, first, count):
    m = D.log2_exact(n)
    assert 2 <= n <= big_n // 4 and count >= 1 and first + count <= m
    return m


def diagonal_indices(n, first, count):
    """indices mod 2n: on 2n rows the group is never the top one"""
    return D.diagonal_indices(2 * n, first, count)


def diagonal_count(n, first, count):
    return (2 << count) - 1


def table(tables, n, first, count, inverse=False, constant=1.0):
    check(len(tables[1]), n, first, count)
    rows = 2 * n
    base = S.table(tables, rows, first, count, inverse=inverse, constant=constant)
    ds = np.array(diagonal_indices(n, first, count), dtype=np.int64)
    assert base.shape == (diagonal_count(n, first, count), rows, 2)
    row = np.broadcast_to(np.arange(rows, dtype=np.int64)[None, :], (len(ds), rows))
    col = (row + ds[:, None]) & (rows - 1)
    bits = ((1 << count) - 1) << first
    present = ((row ^ col) & ~bits) == 0
    assert np.all((row >= n)[present] == (col >= n)[present])             # no entry crosses row n
    lower = present & (row >= n)
    re, im = base[..., 0], base[..., 1]
    out = np.zeros_like(base)
    if inverse:
        out[..., 0], out[..., 1] = np.where(lower, im, re), np.where(lower, -re, im)
    else:
        out[..., 0], out[..., 1] = np.where(lower, -im, re), np.where(lower, re, im)
    return out


def apply(tab, n, first, count, x_re, x_im):
    """the packed table on a vector of 2n entries"""
    return D.apply(tab, 2 * n, first, count, x_re, x_im)


def coeff_to_slot_group(tables, n, count, u_re, u_im, constant=1.0):
    """the last-applied group: u of n entries -> the real P of 2n entries (and the imaginary part of v + conj(v), which is zero)"""
    v_re, v_im = apply(table(tables, n, 0, count, inverse=True, constant=constant), n, 0, count, np.tile(u_re, 2), np.tile(u_im, 2))
    return v_re + v_re, v_im - v_im


def slot_to_coeff_group(tables, n, count, p_re, p_im, constant=1.0):
    """the first-applied group: P' of 2n entries -> V + rot_n(V), n entries"""
    v_re, v_im = apply(table(tables, n, 0, count, constant=constant), n, 0, count, p_re, p_im)
    w_re, w_im = v_re + np.roll(v_re, -n), v_im + np.roll(v_im, -n)
    assert np.array_equal(w_re[:n], w_re[n:]) and np.array_equal(w_im[:n], w_im[n:])
    return w_re[:n], w_im[:n]


def coeff_to_slot(tables, z_re, z_im, groups, constant):
    """n slots -> P, 2n real entries: constant * [2 Re; 2 Im] of BR(w)"""
    n = len(z_re)
    m = D.log2_exact(n)
    assert sum(groups) == m and len(groups) >= 2
    consts = B._group_constants(constant, len(groups))
    done, re, im = 0, np.asarray(z_re, dtype=np.float64), np.asarray(z_im, dtype=np.float64)
    for g, (count, c) in enumerate(zip(groups, consts)):
        done += count
        first = m - done
        if g == 0:
            er, ei = S.apply(S.table(tables, n, first, count, inverse=True, col_mask=S.MASK_EVEN, constant=c), n, first, count, re, im)
            orr, oi = S.apply(S.table(tables, n, first, count, inverse=True, col_mask=S.MASK_ODD, conjugate=True, constant=c), n, first, count, re, im)
            re, im = er + orr, ei - oi
        elif g == len(groups) - 1:
            re, im = coeff_to_slot_group(tables, n, count, re, im, c)
        else:
            re, im = S.apply(S.table(tables, n, first, count, inverse=True, constant=c), n, first, count, re, im)
    assert not np.any(im)
    return re


def slot_to_coeff(tables, p, groups, constant):
    """P' = [a; b], 2n real entries -> constant * the slots of the coefficients a + i b"""
    n = len(p) // 2
    assert sum(groups) == D.log2_exact(n) and len(groups) >= 2
    consts = B._group_constants(constant, len(groups))
    done = 0
    re, im = np.asarray(p, dtype=np.float64), np.zeros(2 * n)
    for g, (count, c) in enumerate(zip(groups, consts)):
        first = done
        done += count
        if g == 0:
            re, im = slot_to_coeff_group(tables, n, count, re, im, c)
        elif g == len(groups) - 1:
            er, ei = S.apply(S.table(tables, n, first, count, row_mask=S.MASK_EVEN, constant=c), n, first, count, re, im)
            orr, oi = S.apply(S.table(tables, n, first, count, row_mask=S.MASK_ODD, constant=c), n, first, count, re, im)
            re, im = er + orr, ei - oi
        else:
            re, im = S.apply(S.table(tables, n, first, count, constant=c), n, first, count, re, im)
    return re, im


def pipeline(t, n, primes, delta, half_width, degree, double_angles, down_groups, up_groups, weight_scale, tables):
    """sparse_bootstrap_spec.pipeline on the packed path: coefficients t = D p(Y) + q0 I(X) -> the N coefficients of p(Y), and the constants"""
    big_n = len(t)
    slot_count = big_n // 2
    assert 4 <= n <= big_n // 4
    s = slot_count // n
    k = B.plan_constants(primes, delta, half_width, degree, double_angles, down_groups, up_groups, weight_scale)
    q0 = float(primes[0])
    t = np.asarray(t, dtype=np.float64)
    u = np.where(np.arange(big_n) % s == 0, t * float(s), 0.0)            # 2b. sub_sum: s times the Y-part
    x = (u / delta) * (delta / q0)                                        # 3. the relabel D -> q0
    z_re, z_im = E.simd_from_coefficients(x, tables)
    packed = coeff_to_slot(tables, z_re[:n], z_im[:n], down_groups, k["c1"] / float(s))      # 4'. [2 c1 Re; 2 c1 Im] on period 2n
    relabel = k["s1"] / k["part"]                                         # 5'. the same relabel; no sign
    coeffs = B.interpolant(half_width, degree, double_angles)
    reduced = B.eval_mod_scheduled(packed * relabel, half_width, coeffs, double_angles)      # 6'. ONE operand
    o_re, o_im = slot_to_coeff(tables, reduced, up_groups, k["c2"])       # 8'.
    o_re, o_im = o_re * (k["s2"] / delta), o_im * (k["s2"] / delta)       # 9.
    return E.simd_coefficients(np.tile(o_re, s), np.tile(o_im, s), 1.0, tables), k
