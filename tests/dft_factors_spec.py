"""The factored special DFT behind CoeffToSlot / SlotToCoeff for the generator-3 slot order (include/troyn.h, "Factors of the special DFT"), in
numpy: real and imaginary parts are separate float64 arrays and every product, sum and difference is its own numpy operation, one IEEE rounding
each, as in ckks_encode_spec.py.

N is the ring degree, n = N/2 the slot count, m = log2 n, zeta = exp(2 pi i / 2N).  With t the N real coefficients, w_k = t_k + i t_{k+n} and
z_j = t(zeta^(3^j)) the slots, zh_j = z_j (j even) / conj(z_j) (j odd) is an ordinary special FFT on the rotation group (-3)^j:

    zh = L_{m-1} ... L_0 BR w,        BR the bit reversal on m bits,

layer b (0 <= b < m) with lh = 2^b, len = 2 lh, blocks of len rows and tw_b(j) = zeta^(((-3)^j mod 4 len) (2N / 4 len)) for j < lh:
rows (i + j, i + j + lh) of L_b are [[1, tw], [1, -tw]], of L_b^-1 they are 1/2 [[1, 1], [1/tw, -1/tw]].

table(...) is the product of the layers [first, first + count) by its present diagonals, diag_d[i] = M[i][(i + d) mod n]; forward the product is
L_{first+count-1} ... L_first (layer `first` applied first), inverse it is L_first^-1 ... L_{first+count-1}^-1 (the top layer applied first).
An entry M[row][col] is present when row and col agree outside the bits [first, first + count); it is ONE product of butterfly coefficients, in
the order of application, with a fixed association:

    acc = (constant, 0)
    per layer b:  c = the layer's coefficient for (row bit b, col bit b); a coefficient 1 is skipped, otherwise acc = acc * c (four products, one
                  difference, one sum); inverse: then acc = acc * 0.5 (two products), for every layer
        forward   col bit 0: 1      col bit 1: +tw_b(row mod lh) (row bit 0) / -tw_b(row mod lh) (row bit 1)
        inverse   row bit 0: 1      row bit 1: +conj tw_b(col mod lh) (col bit 0) / -conj tw_b(col mod lh) (col bit 1)
    conjugate: acc = (acc.re, -acc.im)

A twiddle is read from the encoder handle's root_powers table only (root_powers[i] = zeta^bitrev(i, log2 N)): zeta^k for k in [0, 2N) is
root_powers[bitrev(k mod N)], negated for k >= N (k mod N is never 0 here); sign and conjugation are exact.  Absent and masked entries are +0.
"""
import numpy as np

from ckks_encode_spec import reverse_bits

MASK_NONE, MASK_EVEN, MASK_ODD = 0, 1, 2


def log2_exact(x):
    b = int(x).bit_length() - 1
    assert x == 1 << b
    return b


def diagonal_indices(n, first, count):
    """the present diagonals of a product of `count` >= 1 layers from `first`, ascending mod n: the multiples of 2^first up to +-(2^count - 1) of them"""
    m = log2_exact(n)
    assert count >= 1 and first + count <= m
    step, reach = 1 << first, 1 << count
    if first + count == m:                       # +k and -(2^count - k) coincide mod n
        return [k * step for k in range(reach)]
    return [k * step for k in range(reach)] + [n - k * step for k in range(reach - 1, 0, -1)]


def diagonal_count(n, first, count):
    return len(diagonal_indices(n, first, count))


def twiddle(roots, log_n, b, j):
    """tw_b(j) from root_powers: (re, im)"""
    big_n = 1 << log_n
    len4 = 1 << (b + 3)
    k = pow(-3, int(j), len4) * (2 * big_n // len4)
    r = roots[reverse_bits(k % big_n, log_n)]
    return (-r[0], -r[1]) if k >= big_n else (r[0], r[1])


def _mul(ar, ai, cr, ci):
    return ar * cr - ai * ci, ar * ci + ai * cr


def entry(tables, first, count, inverse, row, col, constant):
    """M[row][col] of the product, or None where it is absent"""
    _, roots, _ = tables
    log_n = log2_exact(len(roots))
    bits = ((1 << count) - 1) << first
    if (row ^ col) & ~bits:
        return None
    ar, ai = np.float64(constant), np.float64(0.0)
    half = np.float64(0.5)
    order = range(first + count - 1, first - 1, -1) if inverse else range(first, first + count)
    for b in order:
        rb, cb = (row >> b) & 1, (col >> b) & 1
        lh = 1 << b
        if not inverse:
            if cb:
                tr, ti = twiddle(roots, log_n, b, row & (lh - 1))
                if rb:
                    tr, ti = -tr, -ti
                ar, ai = _mul(ar, ai, np.float64(tr), np.float64(ti))
        else:
            if rb:
                tr, ti = twiddle(roots, log_n, b, col & (lh - 1))
                ti = -ti
                if cb:
                    tr, ti = -tr, -ti
                ar, ai = _mul(ar, ai, np.float64(tr), np.float64(ti))
            ar, ai = ar * half, ai * half
    return ar, ai


def _twiddles(roots, log_n, b, j):
    """tw_b(j) for an array of j: (re [..], im [..])"""
    big_n = 1 << log_n
    len4 = 1 << (b + 3)
    powers = np.ones(big_n // 2, dtype=np.int64)                 # (-3)^j mod 2N; 4 len divides 2N
    for x in range(1, len(powers)):
        powers[x] = (powers[x - 1] * -3) % (2 * big_n)
    k = (powers[j] % len4) * (2 * big_n // len4)
    low, idx = k % big_n, np.zeros(j.shape, dtype=np.int64)
    for bit in range(log_n):
        idx |= ((low >> bit) & 1) << (log_n - 1 - bit)
    sign = np.where(k >= big_n, -1.0, 1.0)
    return roots[idx, 0] * sign, roots[idx, 1] * sign          # a product with +-1 is exact


def table(tables, first, count, inverse=False, col_mask=MASK_NONE, row_mask=MASK_NONE, conjugate=False, constant=1.0):
    """float64 [nd][n][2]: the present diagonals of the product, ascending diagonal index mod n (entry() over every row at once)"""
    roots = np.asarray(tables[1], dtype=np.float64)
    log_n = log2_exact(len(roots))
    n = len(roots) // 2
    ds = np.array(diagonal_indices(n, first, count), dtype=np.int64)
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
        tr, ti = _twiddles(roots, log_n, b, (col if inverse else row) & (lh - 1))
        if inverse:
            ti = -ti
        neg = cb if inverse else rb
        tr, ti = np.where(neg, -tr, tr), np.where(neg, -ti, ti)
        pr, pi = _mul(ar, ai, tr, ti)
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
    """the dense product: y[i] = SUM_a tab[a][i] * x[(i + d_a) mod n], summed in ascending a -> (re, im)"""
    ds = diagonal_indices(n, first, count)
    x_re, x_im = np.asarray(x_re, dtype=np.float64), np.asarray(x_im, dtype=np.float64)
    y_re, y_im = np.zeros(n), np.zeros(n)
    for a, d in enumerate(ds):
        rr, ri = np.roll(x_re, -d), np.roll(x_im, -d)
        pr, pi = _mul(tab[a, :, 0], tab[a, :, 1], rr, ri)
        y_re, y_im = y_re + pr, y_im + pi
    return y_re, y_im


def bit_reverse(x, n):
    m = log2_exact(n)
    return np.asarray(x)[[reverse_bits(i, m) for i in range(n)]]


def default_groups(m, at_most=4):
    """near-equal groups of at most `at_most` layers, the larger ones first: the plans' default"""
    g = -(-m // at_most)
    return [m // g + (1 if i < m % g else 0) for i in range(g)]
