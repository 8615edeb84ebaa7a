"""GPU parity of the kernels at the scheme boundary with tests/scheme_boundary_spec.py (Python integers), word for word through the C-ABI:
bfv_scale_up_kernel, bfv_decrypt_round_kernel, plain_centralize_kernel and the centralising NTT loader, bgv_delta_kernel / bgv_finish_kernel,
bgv_decrypt_mod_t_kernel, divide_round_q_last_kernel and troyn_mod_switch_drop.  The parametrisation carries the coverage:

  * scale-up: t from 2^40 - 87 on makes m (Q mod t) wider than one word (the 128-bit path of div128_small_quotient); the last t, and every t
    against the 30-bit chain, is above the primes;
  * centralize: t above q_l (a 40-bit prime and 2^45 over 30-bit limbs, 2^59 over 40-bit limbs), t a multiple of q_l (2 q_0, q_1) and t below q_l;
  * BGV mod switch: t = 2N gives q_last = 1 mod t (bgv_delta_kernel's shortcut), the other t do not;
  * decrypt_mod_t: phases whose double sum is within an ulp or two of a half-integer.

These kernels work coefficient by coefficient, so the rings are N = 64 and N = 1024, plus, on one chain each, the smallest ring whose launch has
two chunks per row: N = 512 for the kernels launched with chunks_single (ceil(N / 256): scale-up, decrypt, centralize, the BGV steps) and N = 1024
for those launched with chunks_pairs (ceil(N / 2 / 256): divide_round_q_last_kernel, the limb copy of mod_switch_drop).  Every call has a batch of 3
distinct items.  What the inputs are is asserted without a GPU in tests/test_scheme_boundary_spec.py."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import scheme_boundary_spec as S
from test_gpu_corners import _patterns

pytestmark = pytest.mark.gpu

N_TWO_CHUNKS = 512           # chunks_single(512) = 2
N_TWO_CHUNKS_PAIRS = 1024    # chunks_pairs(1024) = 2
BATCH = 3


def _cases(chains, two_chunks):
    out = [(tuple(b), n) for b in chains for n in (64, 1024)]
    if two_chunks not in (64, 1024):
        out.append((tuple(chains[0]), two_chunks))
    return out


def _ids(case):
    return "%s-N%d" % ("_".join(str(b) for b in case[0]), case[1])


def _setup(O, pkg, dev, bits, n):
    q = [int(v) for v in O.coeff_modulus_create(n, list(bits))]
    return q, pkg.Plan(dev, n.bit_length() - 1, q)


def _uniform(O, seed, q, n):
    return np.stack([O.fill_uniform(seed * 131 + j, int(qj), n) for j, qj in enumerate(q)])


def _ints(a):
    return [int(v) for v in np.asarray(a).reshape(-1)]


def _ntt(O, x, q, n):
    """the oracle's forward transform of [..][L][n] (L = len(q))"""
    tables = [O.NTTTables(n.bit_length() - 1, int(qj)) for qj in q]
    flat = np.ascontiguousarray(x, dtype=np.uint64).reshape(-1).copy()
    O.ntt_forward(flat, flat.size // (len(q) * n), len(q), n.bit_length() - 1, tables)
    return flat.reshape(np.asarray(x).shape)


def _split(cols, n):
    """[L][BATCH * n] columns -> [BATCH][L][n]"""
    return np.ascontiguousarray(np.stack([cols[:, b * n:(b + 1) * n] for b in range(BATCH)]))


@pytest.mark.parametrize("case", _cases(S.SCALE_UP_CHAINS, N_TWO_CHUNKS), ids=_ids)
def test_scale_up(O, pkg, dev, case):
    """troyn_bfv_scale_up with a plain_coeff_count below N (N - 5) and plaintext rows N + 8 words apart (the words a row does not hold are 2^63: reading
    one shows), from the level of the whole chain and from its first prime alone; plain, negated, add-to-source and subtract-from-source forms."""
    bits, n = case
    q, plan = _setup(O, pkg, dev, bits, n)
    count, stride = n - 5, n + 8
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for t in S.scale_up_plain_moduli():
        for L in sorted({len(q), 1}, reverse=True):
            behz = pkg.Behz(plan, L, t)
            edges = S.scale_up_edges(q[:L], t, S.SEED)
            plain = np.full((BATCH, stride), 1 << 63, dtype=np.uint64)
            for b in range(BATCH):
                plain[b, :count] = O.fill_uniform(40 + b, t, count)
            plain[0, :len(edges)] = edges
            plain[1, count - len(edges):count] = edges
            src = np.stack([_uniform(O, 50 + b, q[:L], n) for b in range(BATCH)])
            d_plain, d_src = pkg.to_device(plain, dev), pkg.to_device(src, dev)
            for with_src in (False, True):
                for subtract in (False, True):
                    out = torch.full((BATCH, L, n), -1, dtype=torch.int64, device=dev)
                    pkg.capi.check(plan.lib.troyn_bfv_scale_up(behz.h, C.c_void_p(d_plain.data_ptr()), count, stride,
                                                               C.c_void_p(d_src.data_ptr()) if with_src else None, L * n,
                                                               C.c_void_p(out.data_ptr()), L * n, int(subtract), BATCH, stream))
                    got = pkg.to_host(out)
                    for b in range(BATCH):
                        want = S.bfv_scale_up(plain[b, :count], q[:L], t, n=n, src=src[b] if with_src else None, subtract=subtract)
                        assert np.array_equal(got[b], want), (t, L, with_src, subtract, b)


@pytest.mark.parametrize("case", _cases(S.SCALE_UP_CHAINS, N_TWO_CHUNKS), ids=_ids)
def test_decrypt_scale_and_round(O, pkg, dev, case):
    """every plain modulus of the scale-up list (the handle's gamma is a 61-bit prime, coprime to all of them) at every level: round_boundaries, then
    scale-ups with noise at both ends of [-Q//(4t), Q//(4t)], then uniform residues.  The GPU is compared with the algorithm's specification;
    where there is room for noise (Q >= 4t) the noisy scale-ups must also come back as the plaintext."""
    bits, n = case
    q, plan = _setup(O, pkg, dev, bits, n)
    for t in S.scale_up_plain_moduli():
        for L in range(len(q), 0, -1):
            behz = pkg.Behz(plan, L, t)
            gamma = behz.gamma
            assert math.gcd(gamma, t) == 1 and gamma >> 60 == 1
            cols = _uniform(O, 60 + L, q[:L], BATCH * n)
            edges = S.residue_rows(S.round_boundaries(q[:L], t, S.SEED), q[:L])
            m = S.scale_up_inputs(q[:L], t, S.SEED, _ints(O.fill_uniform(13, t, n)))
            noisy = S.residue_rows(S.noisy_scale_ups(m, q[:L], t), q[:L])
            cols[:, :edges.shape[1]] = edges
            cols[:, edges.shape[1]:edges.shape[1] + n] = noisy
            phase = _split(cols, n)
            got = pkg.to_host(behz.decrypt_scale_and_round(pkg.to_device(phase, dev)))
            for b in range(BATCH):
                assert _ints(got[b]) == S.bfv_decrypt_scale_and_round(phase[b], q[:L], t, gamma), (t, L, b)
            if S.product(q[:L]) >= 4 * t:
                assert _ints(got.reshape(-1)[edges.shape[1]:edges.shape[1] + n]) == m, (t, L)


def _centralize_inputs(O, q, t, n):
    """[BATCH][n] coefficients below t: the ends, either side of the sign threshold, either side of every q_l and of its multiples next to the
    threshold and to t when t > q_l; uniform otherwise"""
    edges = [0, 1, t - 1, (t - 1) // 2, (t + 1) // 2]
    for ql in q:
        if t > ql:
            for mult in (1, 2, ((t + 1) // 2) // ql, ((t + 1) // 2) // ql + 1, (t - 1) // ql):
                edges += [mult * ql - 1, mult * ql, mult * ql + 1]
    edges = [v for v in S.unique(edges) if 0 <= v < t][:n]
    m = np.stack([O.fill_uniform(70 + b, t, n) for b in range(BATCH)])
    m[0, :len(edges)] = edges
    m[2, n - len(edges):] = edges
    return m


@pytest.mark.parametrize("case", _cases(S.CENTRALIZE_CHAINS, N_TWO_CHUNKS), ids=_ids)
def test_centralize_and_centralize_ntt(O, pkg, dev, case):
    """troyn_plain_centralize and troyn_plain_centralize_ntt (plain_coeff_count N - 3) at every level; the NTT entry against the specification
    followed by the oracle's forward transform.  {30,30,30}: t = a 40-bit prime, 2 q_0, q_1, 2^45 (never below a q_l: the general lift, two
    launches); {60,40,40,60}: t = 2, 2^21 (the fast lift; one launch with the centralising loader from N = 1024 on) and 2^59 (above the 40-bit limbs)."""
    bits, n = case
    q, plan = _setup(O, pkg, dev, bits, n)
    for t in S.centralize_plain_moduli(bits, q):
        m = _centralize_inputs(O, q, t, n)
        dm = pkg.to_device(m, dev)
        for L in range(1, len(q) + 1):
            got = pkg.to_host(plan.plain_centralize(L, t, dm))
            got_ntt = pkg.to_host(plan.plain_centralize_ntt(L, t, dm, coeff_count=n - 3))
            for b in range(BATCH):
                assert np.array_equal(got[b], S.plain_centralize(m[b], q[:L], t)), (t, L, b)
                want = _ntt(O, S.plain_centralize(m[b, :n - 3], q[:L], t, n=n), q[:L], n)
                assert np.array_equal(got_ntt[b], want), (t, L, b, "ntt")


def _bgv_inputs(O, q, t, n):
    """coefficient form [BATCH][2][L][n]: bgv_last_limb_edges at the front of item 0 and at the back of item 1 (both polynomials), corner rows
    (q_j - 1, 0, alternating) under a uniform last limb in item 2; uniform otherwise"""
    L = len(q)
    edges = S.bgv_last_limb_edges(q, t, S.SEED)[:, :n]
    x = np.stack([np.stack([_uniform(O, 80 + 2 * b + p, q, n) for p in range(2)]) for b in range(BATCH)])
    x[0, 0, :, :edges.shape[1]] = edges
    x[0, 1, :, 3:3 + edges.shape[1]] = edges
    x[1, 0, :, n - edges.shape[1]:] = edges
    idx = np.arange(n)
    for j in range(L - 1):
        x[2, 0, j] = np.uint64(q[j] - 1)
        x[2, 1, j] = np.where(idx % 2 == 0, 0, q[j] - 1).astype(np.uint64)
    x[1, 1, :L - 1] = 0
    return x


@pytest.mark.parametrize("case", _cases(S.BGV_CHAINS, N_TWO_CHUNKS), ids=_ids)
def test_bgv_mod_switch(O, pkg, dev, case):
    """troyn_bgv_mod_t_and_divide_q_last_ntt at every level from the whole chain down to 2, t = 2, 2N, 257, 65537, 2^20 and a 49-bit prime: the
    inputs are transformed with the oracle and the result is compared in NTT form.  q_last is invertible mod every t of the list (odd primes
    against powers of two and against primes they differ from), so no level is refused; at t = 2N the inverse is 1."""
    bits, n = case
    q, plan = _setup(O, pkg, dev, bits, n)
    for t in S.bgv_plain_moduli(n):
        for L in range(len(q), 1, -1):
            assert math.gcd(q[L - 1], t) == 1
            bgv = pkg.Bgv(plan, L, t)
            assert bgv.inv_q_last_mod_t == pow(q[L - 1], -1, t) and (bgv.inv_q_last_mod_t == 1) == (q[L - 1] % t == 1) and (t != 2 * n or q[L - 1] % t == 1)
            x = _bgv_inputs(O, q[:L], t, n)
            got = pkg.to_host(bgv.mod_t_and_divide_q_last_ntt(pkg.to_device(_ntt(O, x, q[:L], n), dev), 2))
            for b in range(BATCH):
                for p in range(2):
                    want = _ntt(O, S.bgv_mod_t_and_divide_q_last(x[b, p], q[:L], t), q[:L - 1], n)
                    assert np.array_equal(got[b, p], want), (t, L, b, p)


@pytest.mark.parametrize("n,bits", [(64, [30, 30, 30]), (1024, [50, 50, 50, 50])])
def test_bgv_switch_key_with_unit_inverse(O, pkg, dev, n, bits):
    """the BGV key-switch tail shares the division mod t; at t = 2N the special prime is 1 mod t.  Against the oracle's host key switch (the
    specification module has no key switch), OVERWRITE and ADD_INPLACE, corner and uniform targets."""
    t = 2 * n
    q, plan = _setup(O, pkg, dev, bits, n)
    ctx = O.Context("bgv", n, q, t)
    K = len(q)
    key_level = pkg.Bgv(plan, K, t)
    assert key_level.inv_q_last_mod_t == 1 and ctx.bgv_inv_q_last_mod_t(K) == 1
    for L in range(K - 1, 0, -1):
        keys_h = ctx.random_keys(40 + L, L)
        keys_d = [pkg.to_device(k, dev) for k in keys_h]
        target = np.stack([ctx.random_ct(3 * L + b, 1, L)[0] for b in range(BATCH)])
        target[1] = np.stack([_patterns(q[j], n, 1)["all_q-1"] for j in range(L)])
        old = np.stack([ctx.random_ct(9 * L + b, 2, L) for b in range(BATCH)])
        for assign in (pkg.ASSIGN_OVERWRITE, pkg.ASSIGN_ADD_INPLACE):
            dest = pkg.to_device(old.copy(), dev)
            key_level.switch_key(L, pkg.to_device(target, dev), keys_d, dest=dest, assign=assign)
            got = pkg.to_host(dest)
            for b in range(BATCH):
                assert np.array_equal(got[b], ctx.switch_key(L, True, target[b], keys_h, assign=assign, dest=old[b].copy())), (L, assign, b)


@pytest.mark.parametrize("case", _cases(S.DECRYPT_MOD_T_CHAINS, N_TWO_CHUNKS), ids=_ids)
def test_bgv_decrypt_mod_t(O, pkg, dev, case):
    """troyn_bgv_decrypt_mod_t at every level, correction factors 1 and 3, t = 65537, 2^20, a 49-bit prime and 2^59: half_integer_phases at the
    front of item 0 for L = 2 and 3 (the double sum is a tie or an ulp from one: a reciprocal division, a fused multiply-add or another order of
    the sum changes words here), zeros at the front of item 2, uniform phases otherwise."""
    bits, n = case
    q, plan = _setup(O, pkg, dev, bits, n)
    for t in S.decrypt_mod_t_plain_moduli():
        for L in range(1, len(q) + 1):
            bgv = pkg.Bgv(plan, L, t)
            phase = np.stack([_uniform(O, 90 + b + 3 * L, q[:L], n) for b in range(BATCH)])
            if L in (2, 3):
                half = S.half_integer_phases(q[:L], S.SEED)
                phase[0, :, :half.shape[1]] = half
            phase[2, :, :4] = 0
            d_phase = pkg.to_device(phase, dev)
            for cf in (1, 3):
                got = pkg.to_host(bgv.decrypt_mod_t(d_phase, cf))
                for b in range(BATCH):
                    assert _ints(got[b]) == S.bgv_decrypt_mod_t(phase[b], q[:L], t, cf), (t, L, cf, b)


@pytest.mark.parametrize("case", _cases(S.DIVIDE_CHAINS, N_TWO_CHUNKS_PAIRS), ids=_ids)
def test_divide_and_round_q_last_and_drop(O, pkg, dev, case):
    """troyn_divide_and_round_q_last (coefficient form, pcount 2) and troyn_mod_switch_drop to L - 1 and to 1, at every level: divide_edges (0, 1,
    Q - 1, +-floor(Q/2), X mod q_last in {h-1, h, h+1}) and uniform residues in a batch of 3, then every corner pattern of test_gpu_corners.py
    (15 patterns at N = 1024, 13 at N = 64 where impulse positions coincide, filled up with uniform polynomials to a batch of 8 or 7)."""
    bits, n = case
    q, plan = _setup(O, pkg, dev, bits, n)
    for L in range(len(q), 1, -1):
        edges = S.residue_rows(S.divide_edges(q[:L]), q[:L])[:, :n]
        x = np.stack([np.stack([_uniform(O, 100 + 2 * b + p, q[:L], n) for p in range(2)]) for b in range(BATCH)])
        x[0, 0, :, :edges.shape[1]] = edges
        x[1, 1, :, n - edges.shape[1]:] = edges
        x[2, 0, :, 1:1 + edges.shape[1]] = edges
        names = sorted(_patterns(q[0], n, 1))
        polys = [np.stack([_patterns(q[j], n, 1)[nm] for j in range(L)]) for nm in names] + [_uniform(O, 120, q[:L], n)]
        if len(polys) % 2:
            polys.append(_uniform(O, 121, q[:L], n))
        y = np.stack(polys).reshape(len(polys) // 2, 2, L, n)
        for data in (x, y):
            d = pkg.to_device(data, dev)
            got = pkg.to_host(plan.divide_and_round_q_last(L, d, 2))
            drop_next = pkg.to_host(plan.mod_switch_drop(L, L - 1, d, 2))
            drop_first = pkg.to_host(plan.mod_switch_drop(L, 1, d, 2))
            for b in range(data.shape[0]):
                for p in range(2):
                    assert np.array_equal(got[b, p], S.divide_and_round_q_last(data[b, p], q[:L])), (L, b, p)
                    assert np.array_equal(drop_next[b, p], S.mod_switch_drop(data[b, p], L - 1)), (L, b, p)
                    assert np.array_equal(drop_first[b, p], S.mod_switch_drop(data[b, p], 1)), (L, b, p)
