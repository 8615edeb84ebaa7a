"""The contract of troyn_scalar_weighted_sums (include/troyn.h) in Python big integers.

  out[s][b][c][l][i] = ( SUM_t scalars[s][t][l] * in[t][b][c][l][i]
                         + (c == 0 and (i == 0 or not constant_at_index0) ? constants[s][l] : 0) ) mod q_l      in canonical form

in[t] is [batch][pcount][in_nmod[t]][N] with in_nmod[t] >= nmod = len(moduli); limbs at or beyond nmod are never indexed.
"""
import numpy as np


def _big(x):
    return np.asarray(x, dtype=np.uint64).astype(object)


def scalar_weighted_sums(moduli, inputs, scalars, constants=None, constant_at_index0=False):
    """moduli: the nmod moduli of the output limbs; inputs: list of uint64 arrays [batch][pcount][>= nmod][N]; scalars [slots][terms][nmod];
    constants [slots][nmod] or None.  Returns uint64 [slots][batch][pcount][nmod][N]: ONE reduction, after the whole sum over the integers."""
    nmod, terms, slots = len(moduli), len(inputs), len(scalars)
    batch, pcount, _, n = inputs[0].shape
    big = [_big(x[:, :, :nmod, :]) for x in inputs]
    out = np.zeros((slots, batch, pcount, nmod, n), dtype=np.uint64)
    for s in range(slots):
        for l, q in enumerate(moduli):
            acc = np.zeros((batch, pcount, n), dtype=object)
            for t in range(terms):
                acc = acc + int(scalars[s][t][l]) * big[t][:, :, l, :]
            if constants is not None:
                if constant_at_index0:
                    acc[:, 0, 0] = acc[:, 0, 0] + int(constants[s][l])
                else:
                    acc[:, 0, :] = acc[:, 0, :] + int(constants[s][l])
            out[s, :, :, l, :] = (acc % int(q)).astype(np.uint64)
    return out


def fold_term_by_term(moduli, inputs, scalars, constants=None, constant_at_index0=False):
    """the same value as multiply_scalar + add would form it: every product and every sum reduced at once"""
    nmod, terms, slots = len(moduli), len(inputs), len(scalars)
    batch, pcount, _, n = inputs[0].shape
    out = np.zeros((slots, batch, pcount, nmod, n), dtype=np.uint64)
    for s in range(slots):
        for l, q in enumerate(moduli):
            q = int(q)
            acc = np.zeros((batch, pcount, n), dtype=object)
            for t in range(terms):
                prod = (int(scalars[s][t][l]) * _big(inputs[t][:, :, l, :])) % q
                acc = (acc + prod) % q
            if constants is not None:
                c = np.zeros((batch, pcount, n), dtype=object)
                if constant_at_index0:
                    c[:, 0, 0] = int(constants[s][l])
                else:
                    c[:, 0, :] = int(constants[s][l])
                acc = (acc + c) % q
            out[s, :, :, l, :] = acc.astype(np.uint64)
    return out
