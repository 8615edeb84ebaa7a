"""Specification of the BFV inner product, composed from the oracle's bare tools (no GPU, no library code):

    out = floor_step( INTT( SUM_t NTT(lift(a_t)) (x) NTT(lift(b_t)) ) )

lift = fast_b_conv_m_tilde, sm_mrq and the forward transforms in q and in Bsk (steps (1)-(3) of the reference's Evaluator::bfv_multiply),
(x) the two-by-two tensor product with products and sums modulo each prime in Python integers, floor_step = multiply by t, fast_floor,
fast_b_conv_sk (steps (6)-(8)).  It works in the reference's 61-bit auxiliary base."""
import numpy as np


class BfvDotSpec:
    def __init__(self, O, n, q, L, t):
        self.O, self.n, self.L, self.t = O, n, L, t
        self.log_n = n.bit_length() - 1
        self.q = [int(p) for p in q[:L]]
        self.tool = O.RNSTool(n, self.q, t)
        self.bsk = self.tool.base_Bsk
        self.S = len(self.bsk)
        self.q_tables = [O.NTTTables(self.log_n, p) for p in self.q]
        self.bsk_tables = [O.NTTTables(self.log_n, p) for p in self.bsk]
        self.primes = self.q + self.bsk

    def lift(self, ct):
        """ct [2][L][N] coefficient form -> object array [2][L + S][N] of NTT-form residues (rows of q, then rows of Bsk)"""
        O, n, L, S = self.O, self.n, self.L, self.S
        ct = np.ascontiguousarray(ct, dtype=np.uint64).reshape(2, L, n)
        in_q = ct.copy().reshape(-1)
        O.ntt_forward(in_q, 2, L, self.log_n, self.q_tables)
        in_b = np.concatenate([self.tool.sm_mrq(self.tool.fast_b_conv_m_tilde(ct[i].reshape(-1))) for i in range(2)])
        O.ntt_forward(in_b, 2, S, self.log_n, self.bsk_tables)
        return np.concatenate([in_q.reshape(2, L, n), in_b.reshape(2, S, n)], axis=1).astype(object)

    def tensor(self, la, lb):
        """two lifted operands -> object array [3][L + S][N]: d0 = a0 b0, d1 = a0 b1 + a1 b0, d2 = a1 b1 modulo each prime"""
        d = np.empty((3, self.L + self.S, self.n), dtype=object)
        for r, p in enumerate(self.primes):
            d[0, r] = la[0, r] * lb[0, r] % p
            d[1, r] = (la[0, r] * lb[1, r] + la[1, r] * lb[0, r]) % p
            d[2, r] = la[1, r] * lb[1, r] % p
        return d

    def add(self, x, y):
        out = np.empty_like(x)
        for r, p in enumerate(self.primes):
            out[:, r] = (x[:, r] + y[:, r]) % p
        return out

    def scale(self, x, k):
        out = np.empty_like(x)
        for r, p in enumerate(self.primes):
            out[:, r] = x[:, r] * (k % p) % p
        return out

    def finish(self, d):
        """NTT-form sum [3][L + S][N] -> [3][L][N]: inverse transforms, multiply by t, fast_floor, fast_b_conv_sk"""
        O, n, L, S = self.O, self.n, self.L, self.S
        d_q = np.ascontiguousarray(d[:, :L].astype(np.uint64)).reshape(-1)
        d_b = np.ascontiguousarray(d[:, L:].astype(np.uint64)).reshape(-1)
        O.ntt_inverse(d_q, 3, L, self.log_n, self.q_tables)
        O.ntt_inverse(d_b, 3, S, self.log_n, self.bsk_tables)
        rows = np.concatenate([d_q.reshape(3, L, n), d_b.reshape(3, S, n)], axis=1).astype(object)
        out = np.empty((3, L, n), dtype=np.uint64)
        for i in range(3):
            for r, p in enumerate(self.primes):
                rows[i, r] = rows[i, r] * (self.t % p) % p
            floor = self.tool.fast_floor(np.ascontiguousarray(rows[i].astype(np.uint64)).reshape(-1))
            out[i] = self.tool.fast_b_conv_sk(floor).reshape(L, n)
        return out

    def dot(self, a_list, b_list):
        """SUM_t a_list[t] x b_list[t], every operand [2][L][N]; equal objects are lifted once"""
        lifted = {}

        def lift(x):
            if id(x) not in lifted:
                lifted[id(x)] = self.lift(x)
            return lifted[id(x)]
        acc = None
        for a, b in zip(a_list, b_list):
            d = self.tensor(lift(a), lift(b))
            acc = d if acc is None else self.add(acc, d)
        return self.finish(acc)

    def repeated(self, a, b, terms):
        """the same pair `terms` times: the one-pair tensor product scaled by `terms` before the floor"""
        return self.finish(self.scale(self.tensor(self.lift(a), self.lift(b)), terms))
