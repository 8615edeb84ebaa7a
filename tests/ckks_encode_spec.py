"""The CKKS encoder's contract (include/troyn.h, "CKKS encoder on the device") in numpy and Python integers.

Real and imaginary parts are separate float64 arrays and every product, sum and difference is its own numpy operation: one IEEE
rounding each, in the order and association of CKKSEncoder::encode_complex64_simd / decode_complex64_simd (troy/troy.cpp).  Residues
and the CRT composition use Python integers; float(int) rounds correctly (nearest, ties to even).  The functions take the tables
(index_map [N], root_powers [N][2], inv_root_powers [N][2]) as arguments and work on coefficient-form residues: the NTT is not theirs.
"""
import numpy as np


def reverse_bits(x, bits):
    r = 0
    for _ in range(bits):
        r = (r << 1) | (x & 1)
        x >>= 1
    return r


def index_map_formula(log_n):
    """slot i sits at bitrev((3^i mod 2N - 1) / 2), its conjugate at bitrev((2N - 3^i mod 2N - 1) / 2)"""
    n = 1 << log_n
    m, slots = 2 * n, n // 2
    out = np.zeros(n, dtype=np.uint32)
    pos = 1
    for i in range(slots):
        out[i] = reverse_bits((pos - 1) >> 1, log_n)
        out[i + slots] = reverse_bits((m - pos - 1) >> 1, log_n)
        pos = (pos * 3) & (m - 1)
    return out


def numpy_tables(log_n):
    """the tables from numpy's cos / sin (the library's come from libm: within an ulp, not necessarily equal)"""
    n = 1 << log_n
    m = 2 * n

    def root(k):
        ang = 2.0 * 3.14159265358979323846264338327950288 * float(k % m) / float(m)
        return np.cos(ang), np.sin(ang)
    roots, inv_roots = np.zeros((n, 2)), np.zeros((n, 2))
    for i in range(1, n):
        roots[i] = root(reverse_bits(i, log_n))
        c, s = root(reverse_bits(i - 1, log_n) + 1)
        inv_roots[i] = (c, -s)
    return index_map_formula(log_n), roots, inv_roots


def _layer(a_re, a_im, roots, root_index, mm, gap, decode):
    """one radix-2 layer over mm groups of 2 * gap points; group i uses roots[root_index + i]"""
    re, im = a_re.reshape(mm, 2, gap), a_im.reshape(mm, 2, gap)
    rr, ri = roots[root_index:root_index + mm, 0][:, None], roots[root_index:root_index + mm, 1][:, None]
    ur, ui, wr, wi = re[:, 0, :].copy(), im[:, 0, :].copy(), re[:, 1, :].copy(), im[:, 1, :].copy()
    if decode:      # Cooley-Tukey: v = w * r; (u + v, u - v)
        vr = wr * rr - wi * ri
        vi = wr * ri + wi * rr
        re[:, 0, :], im[:, 0, :], re[:, 1, :], im[:, 1, :] = ur + vr, ui + vi, ur - vr, ui - vi
    else:           # Gentleman-Sande: (u + v, (u - v) * r)
        dr, di = ur - wr, ui - wi
        re[:, 0, :], im[:, 0, :] = ur + wr, ui + wi
        re[:, 1, :], im[:, 1, :] = dr * rr - di * ri, dr * ri + di * rr


def simd_coefficients(values_re, values_im, scale, tables):
    """encode_complex64_simd up to the scaled real coefficients: float64 [N]"""
    index_map, _, inv_roots = tables
    n = len(index_map)
    count = len(values_re)
    assert count <= n // 2
    a_re, a_im = np.zeros(n), np.zeros(n)
    vr, vi = np.asarray(values_re, dtype=np.float64), np.asarray(values_im, dtype=np.float64)
    a_re[index_map[:count]], a_im[index_map[:count]] = vr, vi
    a_re[index_map[n // 2:n // 2 + count]], a_im[index_map[n // 2:n // 2 + count]] = vr, -vi
    root_index, mm, gap = 1, n // 2, 1
    while mm >= 1:
        _layer(a_re, a_im, inv_roots, root_index, mm, gap, False)
        root_index += mm
        mm, gap = mm // 2, gap * 2
    return a_re * (scale / float(n))


def polynomial_coefficients(coeffs, scale, n):
    out = np.zeros(n)
    c = np.asarray(coeffs, dtype=np.float64)
    out[:len(c)] = c * scale
    return out


def residues(coefficients, moduli):
    """set_plaintext: round half to even, reduce the integer modulo every prime -> (uint64 [L][N], too_large)"""
    v = np.rint(coefficients)
    too_large = bool(np.any(np.abs(v) >= 2.0 ** 128))
    out = np.zeros((len(moduli), len(v)), dtype=np.uint64)
    if too_large:
        return out, True
    ints = [int(x) for x in v]
    for i, q in enumerate(moduli):
        out[i] = [x % q for x in ints]          # Python's % is the canonical residue of a negative integer too
    return out, False


def compose(res, moduli):
    """coefficient-form residues [L][N] -> the centred representatives in (-Q/2, Q/2] as Python integers"""
    L, n = len(moduli), res.shape[1]
    Q = 1
    for q in moduli:
        Q *= q
    punctured = [Q // q for q in moduli]
    inv = [pow(p % q, -1, q) for p, q in zip(punctured, moduli)]
    out = []
    for j in range(n):
        x = sum(int(res[i][j]) * inv[i] % moduli[i] * punctured[i] for i in range(L)) % Q
        out.append(x - Q if 2 * x > Q else x)
    return out


def polynomial_from_residues(res, moduli, scale):
    """decode_float64_polynomial: the centred integer correctly rounded to double, divided by the scale"""
    return np.array([float(x) for x in compose(res, moduli)], dtype=np.float64) / np.float64(scale)


def simd_from_coefficients(coefficients, tables):
    """the Cooley-Tukey layers of decode_complex64_simd and the slot gather -> (re [N/2], im [N/2])"""
    index_map, roots, _ = tables
    n = len(index_map)
    a_re, a_im = np.array(coefficients, dtype=np.float64), np.zeros(n)
    root_index, mm, gap = 1, 1, n // 2
    while mm < n:
        _layer(a_re, a_im, roots, root_index, mm, gap, True)
        root_index += mm
        mm, gap = mm * 2, gap // 2
    return a_re[index_map[:n // 2]], a_im[index_map[:n // 2]]


def round_trip_bound(n, scale, values_abs_sum):
    """|decode(encode(z)) - z| per slot: coefficient rounding N / (2 scale) plus transform error 8 log2(N) 2^-52 sum |z_i|"""
    return n / (2.0 * scale) + 8.0 * np.log2(n) * 2.0 ** -52 * values_abs_sum
