"""Specification of the steps between the stages of the CKKS bootstrap (troy/bootstrap.h; include/troyn.h "Real and imaginary parts of CKKS slots"),
in Python integers and float64.  No GPU.

mu_vector     the forward negacyclic transform of X^(N/2) from a modulus and its root: iota = psi^(N/2) on the lower half, q - iota on the upper half.
              Why the halves: the first Cooley-Tukey layer pairs index j with j + N/2 and sends (0, 1) at (0, N/2) to (+iota, -iota); every later
              layer works inside one half, where the only non-zero entry sits at the head of its block and is copied, never multiplied.
split_rows    s = a + b, d = mu (b - a);  join_rows  out = a + mu b  (mod q, canonical)
interpolant   the Chebyshev coefficients exactly as Evaluator::eval_mod builds them; eval_mod the function it evaluates, in float64
plan_constants  the scales troy::BootstrapPlan expects the evaluator to track, and its constants c1 and c2
pipeline      t = D m + q0 I  ->  m, the whole chain of Evaluator::bootstrap on plaintext coefficients: the relabel to q0, CoeffToSlot by the factored
              DFT of tests/dft_factors_spec.py in the plan's groups with c1 (masked boundary group and its conjugated twin), the split with the sign
              (-1)^j by slot POSITION on the bit-reversed content, the relabel to 2 c1 s1, EvalMod on the schedule of tests/chebyshev_spec.py, the
              join, SlotToCoeff with c2, the scale set to D.
"""
import math

import numpy as np
from numpy.polynomial import chebyshev as npcheb

import chebyshev_spec as C
import ckks_encode_spec as E
import dft_factors_spec as D


def iota_of(n, q, root):
    """psi^(N/2): the square root of -1 modulo q that the root table holds at index 1 = bit_reverse(N/2)"""
    iota = pow(root, n // 2, q)
    assert iota * iota % q == q - 1
    return iota


def mu_vector(n, q, iota):
    return [iota] * (n // 2) + [q - iota] * (n // 2)


def monomial_transform_direct(n, q, root):
    """X^(N/2) at the roots in the transform's output order: index i holds the evaluation at psi^(2 bit_reverse(i) + 1)"""
    bits = n.bit_length() - 1
    out = []
    for i in range(n):
        r = int(format(i, "0%db" % bits)[::-1], 2) if bits else 0
        out.append(pow(root, (2 * r + 1) * (n // 2), q))
    return out


def split_rows(a, b, mu, q):
    return [(x + y) % q for x, y in zip(a, b)], [m * (y - x) % q for x, y, m in zip(a, b, mu)]


def join_rows(a, b, mu, q):
    return [(x + m * y) % q for x, y, m in zip(a, b, mu)]


def interpolant(half_width, degree, double_angles):
    """Evaluator::eval_mod: cos(2 pi (K y - 1/4) / 2^r) on the degree + 1 Chebyshev nodes, the same sums in the same order"""
    nodes = degree + 1
    div = math.ldexp(1.0, double_angles)
    f = [math.cos(2.0 * math.pi * (half_width * math.cos(math.pi * (t + 0.5) / nodes) - 0.25) / div) for t in range(nodes)]
    coeffs = []
    for j in range(nodes):
        s = 0.0
        for t in range(nodes):
            s += f[t] * math.cos(math.pi * j * (t + 0.5) / nodes)
        coeffs.append(s * (1.0 if j == 0 else 2.0) / nodes)
    return coeffs


def eval_mod(x, half_width, degree, double_angles, coeffs=None):
    """sin(2 pi x) / (2 pi) as eval_mod computes it: the interpolant at x / K, r double angles, the factor 1 / (2 pi)"""
    c = interpolant(half_width, degree, double_angles) if coeffs is None else coeffs
    v = npcheb.chebval(np.asarray(x, dtype=np.float64) / half_width, c)
    for _ in range(double_angles):
        v = 2.0 * v * v - 1.0
    return v / (2.0 * math.pi)


def interpolant_error(half_width, degree, double_angles, points=200001):
    """sup-norm distance of the interpolant from cos(2 pi (K y - 1/4) / 2^r) on a fine grid of [-1, 1]"""
    y = np.linspace(-1.0, 1.0, points)
    exact = np.cos(2.0 * math.pi * (half_width * y - 0.25) / math.ldexp(1.0, double_angles))
    return float(np.max(np.abs(npcheb.chebval(y, interpolant(half_width, degree, double_angles)) - exact)))


def plan_constants(primes, delta, half_width, degree, double_angles, down_groups, up_groups, weight_scale):
    """troy::BootstrapPlan: the scales the evaluator tracks through the chain and the two constants (troy/bootstrap.h, steps 3 to 8).
    primes: the data primes as floats, q0 first.  -> dict(c1, c2, s1, part, s_e, s2, levels)"""
    q = [float(p) for p in primes]
    depth = C.total_depth(degree) + double_angles
    gc, gs = len(down_groups), len(up_groups)
    Ld = len(q)
    L1 = Ld - gc
    L2 = L1 - depth
    assert L2 - gs >= 1
    s1 = q[0]                                                  # the relabel to q0: the coefficients read t / q0
    for g in range(gc):
        s1 = s1 * weight_scale / q[Ld - 1 - g]
    c1 = q[L1 - 1] / (2.0 * half_width * s1)                   # EvalMod's working scale becomes the prime it first divides by
    part = s1 * (2.0 * c1)
    s = part * half_width
    for i in range(double_angles):
        s = s * s / q[L1 - (depth - double_angles) - 1 - i]
    s_e = s * (2.0 * math.pi)
    s2 = s_e
    for g in range(gs):
        s2 = s2 * weight_scale / q[L2 - 1 - g]
    return {"c1": c1, "c2": q[0] / s2, "s1": s1, "part": part, "s_e": s_e, "s2": s2, "levels": gc + depth + gs}


def _group_constants(constant, groups):
    root = abs(constant) ** (1.0 / groups)
    return [(-root if g == 0 and constant < 0 else root) for g in range(groups)]


def coeff_to_slot(tables, z_re, z_im, groups, constant):
    """troy::CoeffToSlotPlan on slot values: group by group from the top layer down, inverse layers, the groups-th root of the constant in each; the first
    group is (G E) z + conj(conj(G O) z).  -> constant * BR(w), w_k = t_k + i t_{k+n}"""
    n = len(z_re)
    m = D.log2_exact(n)
    done, re, im = 0, np.asarray(z_re, dtype=np.float64), np.asarray(z_im, dtype=np.float64)
    for g, (count, c) in enumerate(zip(groups, _group_constants(constant, len(groups)))):
        done += count
        first = m - done
        if g == 0:
            er, ei = D.apply(D.table(tables, first, count, inverse=True, col_mask=D.MASK_EVEN, constant=c), n, first, count, re, im)
            orr, oi = D.apply(D.table(tables, first, count, inverse=True, col_mask=D.MASK_ODD, conjugate=True, constant=c), n, first, count, re, im)
            re, im = er + orr, ei - oi
        else:
            re, im = D.apply(D.table(tables, first, count, inverse=True, constant=c), n, first, count, re, im)
    return re, im


def slot_to_coeff(tables, y_re, y_im, groups, constant):
    """troy::SlotToCoeffPlan: from layer 0 up, forward layers; the last group is (E G') y + conj((O G') y)"""
    n = len(y_re)
    done, re, im = 0, np.asarray(y_re, dtype=np.float64), np.asarray(y_im, dtype=np.float64)
    for g, (count, c) in enumerate(zip(groups, _group_constants(constant, len(groups)))):
        first = done
        done += count
        if g == len(groups) - 1:
            er, ei = D.apply(D.table(tables, first, count, row_mask=D.MASK_EVEN, constant=c), n, first, count, re, im)
            orr, oi = D.apply(D.table(tables, first, count, row_mask=D.MASK_ODD, constant=c), n, first, count, re, im)
            re, im = er + orr, ei - oi
        else:
            re, im = D.apply(D.table(tables, first, count, constant=c), n, first, count, re, im)
    return re, im


def eval_mod_scheduled(x, half_width, coeffs, double_angles):
    """eval_mod on the schedule of tests/chebyshev_spec.py (ladder, leaves, recombination), then the double angles and 1 / (2 pi)"""
    v = C.evaluate(np.asarray(x, dtype=np.float64) / half_width, list(coeffs))
    for _ in range(double_angles):
        v = 2.0 * v * v - 1.0
    return v / (2.0 * math.pi)


def pipeline(t, primes, delta, half_width, degree, double_angles, down_groups, up_groups, weight_scale, tables):
    """coefficients t = D m + q0 I (float64) -> the coefficients m, by the steps of Evaluator::bootstrap with the plan's constants and relabels.
    A value travels with the scale it is read at: relabelling the scale from a to b multiplies the value by a / b."""
    k = plan_constants(primes, delta, half_width, degree, double_angles, down_groups, up_groups, weight_scale)
    q0 = float(primes[0])
    n = len(t) // 2
    x = (np.asarray(t, dtype=np.float64) / delta) * (delta / q0)          # 3. the relabel D -> q0: x = D m / q0 + I
    z_re, z_im = E.simd_from_coefficients(x, tables)                      # the slots the raised ciphertext holds
    w_re, w_im = coeff_to_slot(tables, z_re, z_im, down_groups, k["c1"])  # 4. c1 BR(x_k + i x_{k+n}), at the scale s1
    sign = np.where(np.arange(n) % 2 == 0, 1.0, -1.0)                     # X^(N/2) in slot POSITION j: i (-1)^j, whatever the slot holds
    re2 = 2.0 * w_re                                                      # 5. w + conj(w)
    ims = sign * 2.0 * w_im                                               #    (conj(w) - w) i (-1)^j = (-2i Im w) i (-1)^j
    relabel = k["s1"] / k["part"]                                         #    both halves read at 2 c1 s1
    coeffs = interpolant(half_width, degree, double_angles)
    re = eval_mod_scheduled(re2 * relabel, half_width, coeffs, double_angles)      # 6. at the scale s_e
    im = eval_mod_scheduled(ims * relabel, half_width, coeffs, double_angles)
    y_re, y_im = re, sign * im                                            # 7. re + im i (-1)^j
    o_re, o_im = slot_to_coeff(tables, y_re, y_im, up_groups, k["c2"])    # 8. c2 D / q0 z, at the scale s2
    o_re, o_im = o_re * (k["s2"] / delta), o_im * (k["s2"] / delta)       # 9. the scale is set to D
    return E.simd_coefficients(o_re, o_im, 1.0, tables), k
