"""The specification of LinearTransform (troy/linear_transform.h) and troyn_ckks_encode_diagonals (include/troyn.h), numpy only.

A complex n x n matrix M is held by its diagonals, diag_k[i] = M[i][(i + k) mod n].  With the project's rotation rot_s(x)[i] = x[(i + s) mod n]:

    M x = SUM_k diag_k (.) rot_k(x) = SUM_G rot_G( SUM_B w[G][B] (.) rot_B(x) ),      w[G][B][i] = diag_{G+B}[(i - G) mod n]

The split: n1 = baby_count, or the smallest power of two >= sqrt(n) when that is 0; the baby steps are the distinct k mod n1, the giant steps the distinct
k - k mod n1 over the present diagonals k, both ascending; the weight of (G, B) is diagonal G + B with shift s = G.

The device encodes item t from two words (a_t, s_t): slot i (0 <= i < N/2) of the item takes
    diagonals mode   diags[a_t][(i - s_t) mod n]                       (diags [nd][n]: a_t is the row of the table)
    matrix mode      matrix[j][(j + a_t) mod n], j = (i - s_t) mod n    (a_t is the diagonal index)
"""
import numpy as np


def diagonals_of(M):
    """{k: diag_k} for every k in [0, n): diag_k[i] = M[i][(i + k) mod n]"""
    M = np.asarray(M)
    n = M.shape[0]
    i = np.arange(n)
    return {k: M[i, (i + k) % n].copy() for k in range(n)}


def default_baby_count(n):
    n1 = 1
    while n1 * n1 < n:
        n1 *= 2
    return n1


def split(present, n, baby_count=0):
    """(baby_steps, giant_steps) of the present diagonal indices"""
    n1 = baby_count or default_baby_count(n)
    assert n1 & (n1 - 1) == 0 and 0 < n1 <= n
    assert all(0 <= k < n for k in present)
    return sorted({k % n1 for k in present}), sorted({k - k % n1 for k in present})


def rotation_steps(present, n, baby_count=0):
    """the non-zero baby and giant steps, sorted: the Galois keys a transform needs"""
    babies, giants = split(present, n, baby_count)
    return sorted((set(babies) | set(giants)) - {0})


def pairs(present, n, baby_count=0, matrix=False):
    """(where, pairs): where[t] = (g, b), the place of item t in weights[g][b]; pairs[t] = (a_t, s_t).  Giant-major, absent G + B left out.
    a_t is the row of the diagonal table (the position of G + B among the sorted present indices), or G + B itself in matrix mode."""
    present = sorted(present)
    babies, giants = split(present, n, baby_count)
    where, out = [], []
    for g, G in enumerate(giants):
        for b, B in enumerate(babies):
            if G + B in present:
                where.append((g, b))
                out.append((G + B if matrix else present.index(G + B), G))
    return where, np.array(out, dtype=np.uint32).reshape(-1, 2)


def values_of(src, pairs, n, N, matrix):
    """complex [items][N/2]: what troyn_ckks_encode_diagonals encodes.  src: complex [nd][n] (diagonals) or [n][n] (matrix)"""
    src = np.asarray(src)
    i = np.arange(N // 2)
    out = np.empty((len(pairs), N // 2), dtype=np.complex128)
    for t, (a, s) in enumerate(np.asarray(pairs).tolist()):
        j = (i - s) % n
        out[t] = src[j, (j + a) % n] if matrix else src[a, j]
    return out


def rot(x, s):
    """rot_s(x)[i] = x[(i + s) mod n]"""
    return np.roll(x, -s)


def bsgs_apply(diagonals, n, x, baby_count=0):
    """SUM_G rot_G( SUM_B w[G][B] (.) rot_B(x) ) in floating point, built from the split, the pairs and values_of (N/2 = n: no repetition)"""
    present = sorted(diagonals)
    babies, giants = split(present, n, baby_count)
    where, pr = pairs(present, n, baby_count)
    w = values_of(np.stack([diagonals[k] for k in present]), pr, n, 2 * n, False)
    inner = [np.zeros(n, dtype=np.complex128) for _ in giants]
    for t, (g, b) in enumerate(where):
        inner[g] = inner[g] + w[t] * rot(x, babies[b])
    return sum(rot(inner[g], G) for g, G in enumerate(giants))
