"""Specification of troyn_sample_ternary_sparse (include/troyn.h) in numpy: from the generator's word stream w[N] and the Hamming weight h
to the ternary polynomial.

    key_j   = (w_j & ~0xFFFF) | j           48 random bits above the index: distinct, so the order needs no tie rule
    support = the h coefficients with the smallest keys  (argsort(key)[:h])
    sign_j  = bit 0 of w_j                  0 -> +1, 1 -> -1 (stored as q_i - 1)

The stream: word w_j is word j & 1 of AES-CTR block counter + (j >> 1) -- what the oracle's generator hands out as fill_uint64s(N).  words() reads it there;
centered_binomial_from_words() re-derives the oracle's own centred binomial sampler from the same words, which pins the block-to-word order of this file
to the project's (tests/test_sparse_secret_spec.py).
"""
import numpy as np


def words(O, seed_low, seed_high, counter, n):
    """w[n]: the n words an oracle generator (seed, at block `counter`) yields next; n/2 blocks.  Returns (w, the generator, advanced)."""
    rng = O.Rng(seed_low, seed_high)
    for _ in range(counter):
        rng.sample_uint64()                         # one block each
    w = np.zeros(n, dtype=np.uint64)
    O.lib().orc_rng_fill_uint64s(rng.h, O.ptr(w), n)
    return w, rng


def _popcount(x):
    x = x.astype(np.uint64)
    count = np.zeros(x.shape, dtype=np.int64)
    for bit in range(21):
        count += ((x >> np.uint64(bit)) & np.uint64(1)).astype(np.int64)
    return count


def centered_binomial_from_words(w, q):
    """[len(q)][n]: popcount of bits 0..20 minus popcount of bits 24..44 of each word (csrc/crypto_kernels.hpp cbd_from_u64)"""
    mask = np.uint64((1 << 21) - 1)
    v = _popcount(w & mask) - _popcount((w >> np.uint64(24)) & mask)
    return np.stack([np.where(v >= 0, v, int(qi) + v).astype(np.uint64) for qi in q])


def support_and_signs(w, h):
    n = w.shape[0]
    assert 1 <= h <= n <= 65536
    key = (w & ~np.uint64(0xFFFF)) | np.arange(n, dtype=np.uint64)
    support = np.argsort(key, kind="stable")[:h]
    negative = (w & np.uint64(1)).astype(bool)
    return support, negative


def ternary_sparse(w, h, q):
    """[len(q)][n] uint64: exactly h entries 1 or q_i - 1, the same polynomial under every modulus"""
    support, negative = support_and_signs(w, h)
    out = np.zeros((len(q), w.shape[0]), dtype=np.uint64)
    for i, qi in enumerate(q):
        out[i, support] = np.where(negative[support], np.uint64(int(qi) - 1), np.uint64(1))
    return out
