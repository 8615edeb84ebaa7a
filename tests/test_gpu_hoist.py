"""Hoisted rotations on the GPU (troyn_apply_galois_many / troyn_apply_galois_sum) against the exact big-integer specification of
tests/hoist_spec.py -- never against another GPU path.

Small rings (N = 32 / 64): everything by definition.  N = 8192 / 16384: the specification's negacyclic products and exact rounded
division on Python integers; only the NTT <-> coefficient form conversions of operands use the oracle's transform, which
tests/test_keyswitch_spec.py pins to the by-definition transform (as tests/test_gpu_keyswitch_spec.py)."""
import ctypes as C
import functools

import numpy as np
import pytest

from hoist_spec import finish, inner_products
from ks_spec import negacyclic
from test_keyswitch_spec import _ntt_polys

pytestmark = pytest.mark.gpu

EDGE = lambda qs, h: [h - 1, h, h + 1, 0, 1, qs - 1, qs - h, qs - h - 1, qs - h + 1, qs - 2]


def _ints(a):
    return [[int(v) for v in row] for row in a]


def _solve_boundary(q, L, c1, elements, keys_c, rng):
    """item data with digit 0 = the constant polynomial 1 (which every automorphism fixes): solve the special-prime rows of key (term 0, digit 0)
    so that the SUMMED special-prime component of the inner product sits on the rounding boundary at the first coefficients (make_case's
    construction).  keys_c[t][j] are arrays [2][K][N]; returns P (hoist_spec.inner_products) for the solved keys."""
    K, n = len(q), len(c1[0])
    qs, h = q[-1], q[-1] // 2
    assert [int(v) for v in c1[0][:2]] == [1, 0] and not any(int(v) for v in c1[0][1:])
    for c in range(2):
        keys_c[0][0][c][K - 1][:] = 0
    keys_l = [[[_ints(kj[c]) for c in range(2)] for kj in kt] for kt in keys_c]
    P = inner_products(q, L, _ints(c1), elements, keys_l)
    for c in range(2):
        w = [int(v) for v in rng.integers(0, qs, size=n, dtype=np.uint64)]
        edge = EDGE(qs, h)
        w[:len(edge)] = edge if c == 0 else edge[::-1]
        rest = [0] * n
        for t in range(len(elements)):
            rest = [(x + y) % qs for x, y in zip(rest, P[t][c][K - 1])]
        row = [(x - y) % qs for x, y in zip(w, rest)]
        keys_c[0][0][c][K - 1][:] = np.array(row, dtype=np.uint64)
        # digit 0 of term 0 is the constant 1: its product with the solved row is the row itself
        P[0][c][K - 1] = [(x + y) % qs for x, y in zip(P[0][c][K - 1], row)]
        assert [(x + y) % qs for x, y in zip(rest, row)] == w
    return P


@functools.lru_cache(maxsize=None)
def _small_case(O, n, bits, L, order):
    """two different items, four key sets (one per element), keys and spec inner products shared by every test of this chain"""
    q = O.coeff_modulus_create(n, list(bits))
    if order == "reversed":
        q = sorted(q, reverse=True)
    K = len(q)
    rng = np.random.default_rng(n + L)
    elements = [5, 25, 2 * n - 1, 3]
    items = []
    for b in range(2):
        c0 = np.stack([rng.integers(0, q[l], size=n, dtype=np.uint64) for l in range(L)])
        c1 = np.stack([rng.integers(0, q[l], size=n, dtype=np.uint64) for l in range(L)])
        if b == 0:
            c1[0] = 0
            c1[0, 0] = 1
        items.append((c0, c1))
    keys_c = [[np.stack([np.stack([rng.integers(0, q[k], size=n, dtype=np.uint64) for k in range(K)]) for c in range(2)]) for j in range(L)] for t in range(4)]
    return q, elements, items, keys_c, rng


@pytest.mark.parametrize("n,bits,L,order", [(32, (50, 50, 50, 50), 3, None), (64, (60, 40, 40, 60), 3, None), (32, (50, 50, 50), 2, "reversed")])
@pytest.mark.parametrize("scheme,is_ntt", [("ckks", True), ("bfv", False)])
@pytest.mark.parametrize("terms", [1, 3])
def test_small_rings_by_definition(O, pkg, dev, n, bits, L, order, scheme, is_ntt, terms):
    q, all_elements, items, all_keys, rng = _small_case(O, n, bits, L, order)
    sel = [3] if terms == 1 else [0, 1, 2]           # {3} | {5, 25, 2N - 1}
    elements = [all_elements[i] for i in sel]
    keys_c = [[kj.copy() for kj in all_keys[i]] for i in sel]
    # item 0 sits on the rounding boundary of the SUM; the patched inner products equal the recomputed ones
    P0 = _solve_boundary(q, L, items[0][1], elements, keys_c, np.random.default_rng(terms))
    keys_l = [[[_ints(kj[c]) for c in range(2)] for kj in kt] for kt in keys_c]
    assert P0 == inner_products(q, L, _ints(items[0][1]), elements, keys_l)
    P = [P0, inner_products(q, L, _ints(items[1][1]), elements, keys_l)]
    plan = pkg.Plan(dev, n.bit_length() - 1, q)
    dkeys = [[pkg.to_device(np.stack([_ntt_polys(kj[c], q) for c in range(2)]), dev) for kj in kt] for kt in keys_c]
    form = (lambda x: np.stack([_ntt_polys(np.array(x[c], dtype=np.uint64), q[:L]) for c in range(2)])) if is_ntt else (lambda x: np.array(x, dtype=np.uint64))
    ct = pkg.to_device(np.stack([form(np.stack(it)) for it in items]), dev)
    many = pkg.to_host(plan.apply_galois_many(L, ct, elements, dkeys, is_ckks=(scheme == "ckks"), is_ntt_form=is_ntt))
    summed = pkg.to_host(plan.apply_galois_sum(L, ct, elements, dkeys, is_ckks=(scheme == "ckks"), is_ntt_form=is_ntt))
    assert many.shape == (terms, 2, 2, L, n) and summed.shape == (2, 2, L, n)
    for b in range(2):
        c0 = _ints(items[b][0])
        for t in range(terms):
            assert np.array_equal(many[t, b], form(finish(q, L, c0, elements, P[b], [t]))), ("many", b, t)
        assert np.array_equal(summed[b], form(finish(q, L, c0, elements, P[b], range(terms)))), ("sum", b)


@pytest.mark.parametrize("n,bits,L,is_ntt", [(8192, [40, 40, 40], 2, False),
                                             (8192, [60, 40, 40, 60], 3, True),
                                             (16384, [50] * 6, 5, True)])
def test_kernel_sizes_against_spec(O, pkg, dev, n, bits, L, is_ntt):
    """batch = 8 identical items (groups of four items per workgroup, two groups), terms = 2, elements {5, 2N - 1}; the summed special-prime
    component on the rounding boundary"""
    q = O.coeff_modulus_create(n, bits)
    K = len(q)
    plan = pkg.Plan(dev, n.bit_length() - 1, q)
    rng = np.random.default_rng(78)
    elements = [5, 2 * n - 1]
    c0 = np.stack([rng.integers(0, q[l], size=n, dtype=np.uint64) for l in range(L)])
    c1 = np.stack([rng.integers(0, q[l], size=n, dtype=np.uint64) for l in range(L)])
    c1[0] = 0
    c1[0, 0] = 1
    keys_c = [[np.stack([np.stack([rng.integers(0, q[k], size=n, dtype=np.uint64) for k in range(K)]) for c in range(2)]) for j in range(L)] for t in range(2)]
    P = _solve_boundary(q, L, c1, elements, keys_c, rng)

    def to_ntt_rows(x, rows):        # x [len(rows)][N] under moduli q[rows]; the oracle's transform, conversions only
        out = np.empty_like(x)
        for i, r in enumerate(rows):
            c1x = O.Context("ckks", n, [q[r], q[(r + 1) % K]])
            out[i] = c1x.to_ntt(x[i][None, None], 1, 1)[0, 0]
        return out

    data = list(range(L))
    form = (lambda x: np.stack([to_ntt_rows(np.array(x[c], dtype=np.uint64), data) for c in range(2)])) if is_ntt else (lambda x: np.array(x, dtype=np.uint64))
    dkeys = [[pkg.to_device(np.stack([to_ntt_rows(kj[c], list(range(K))) for c in range(2)]), dev) for kj in kt] for kt in keys_c]
    batch = 8
    ct = pkg.to_device(np.repeat(form(np.stack([c0, c1]))[None], batch, axis=0), dev)
    many = pkg.to_host(plan.apply_galois_many(L, ct, elements, dkeys, is_ckks=is_ntt, is_ntt_form=is_ntt))
    summed = pkg.to_host(plan.apply_galois_sum(L, ct, elements, dkeys, is_ckks=is_ntt, is_ntt_form=is_ntt))
    c0l = _ints(c0)
    exp_many = [form(finish(q, L, c0l, elements, P, [t])) for t in range(2)]
    exp_sum = form(finish(q, L, c0l, elements, P, range(2)))
    for i in (0, 3, 7):
        for t in range(2):
            assert np.array_equal(many[t, i], exp_many[t]), ("many", t, i)
        assert np.array_equal(summed[i], exp_sum), ("sum", i)


def test_accumulator_range(O, pkg, dev):
    """22 terms x 3 digits = 66 products per output word, every digit q_j - 1 and every key word m - 1 (one key buffer shared by all terms):
    the accumulator is reduced once per term and never runs across terms"""
    n, L, terms = 1024, 3, 22
    q = O.coeff_modulus_create(n, [60, 60, 60, 60])
    K = len(q)
    plan = pkg.Plan(dev, 10, q)
    elements = [3 + 2 * t for t in range(terms)]
    key_ntt = np.stack([np.stack([np.full(n, q[k] - 1, dtype=np.uint64) for k in range(K)]) for c in range(2)])
    # the transform of a constant polynomial is that constant at every point: the key in coefficient form is (m - 1) at X^0
    key_c = [[[q[k] - 1] + [0] * (n - 1) for k in range(K)] for c in range(2)]
    rng = np.random.default_rng(9)
    c0 = np.stack([rng.integers(0, q[l], size=n, dtype=np.uint64) for l in range(L)])
    c1 = np.stack([np.full(n, q[l] - 1, dtype=np.uint64) for l in range(L)])
    P = inner_products(q, L, _ints(c1), elements, [[key_c] * L] * terms)
    dkey = pkg.to_device(key_ntt, dev)
    ct = pkg.to_device(np.stack([c0, c1])[None], dev)
    keys = [[dkey] * L] * terms
    summed = pkg.to_host(plan.apply_galois_sum(L, ct, elements, keys, is_ckks=False, is_ntt_form=False))
    assert np.array_equal(summed[0], np.array(finish(q, L, _ints(c0), elements, P, range(terms)), dtype=np.uint64))
    many = pkg.to_host(plan.apply_galois_many(L, ct, elements, keys, is_ckks=False, is_ntt_form=False))
    for t in (0, 7, terms - 1):
        assert np.array_equal(many[t, 0], np.array(finish(q, L, _ints(c0), elements, P, [t]), dtype=np.uint64)), t


def test_errors(O, pkg, dev):
    import torch
    n, L = 32, 2
    q = O.coeff_modulus_create(n, [40, 40, 40])
    plan = pkg.Plan(dev, 5, q)
    lib = pkg.capi.lib()
    ctx = O.Context("ckks", n, q)
    ct = pkg.to_device(ctx.random_ct(1, 2, L)[None], dev)
    key = [pkg.to_device(k, dev) for k in ctx.random_keys(2, L)]
    INVALID = pkg.capi.TroynInvalidArgument
    for fn in (plan.apply_galois_many, plan.apply_galois_sum):
        with pytest.raises(INVALID):
            fn(L, ct, [], [])                                   # terms == 0
        for bad in (4, 2 * n, 2 * n + 1, 1):                    # even, >= 2N, the identity
            with pytest.raises(INVALID):
                fn(L, ct, [3, bad], [key, key])
        with pytest.raises(INVALID):
            fn(L, ct, [3], [[key[0], None]])                    # a null entry
        with pytest.raises(INVALID):
            fn(3, pkg.to_device(np.zeros((1, 2, 3, n), dtype=np.uint64), dev), [3], [key + key])      # L = K
        with pytest.raises(INVALID):
            fn(L, ct, [3], [key], out=ct)                       # out overlapping ct
        assert fn(L, ct[:0], [3], [key]).numel() == 0           # batch == 0: TROYN_OK, nothing launched
    # the raw entries: null tables, L = 0, a short workspace
    ws = torch.empty(lib.troyn_apply_galois_hoisted_workspace_bytes(plan.h, L, 1, 1, 1), dtype=torch.uint8, device=dev)
    out = torch.empty_like(ct)
    el = (C.c_uint64 * 1)(3)
    kp = (C.c_void_p * L)(*[k.data_ptr() for k in key])
    args = lambda L_=L, ct_=ct.data_ptr(), el_=el, kp_=kp, out_=out.data_ptr(), wsb=None: (
        plan.h, L_, 1, 1, C.c_void_p(ct_), el_, kp_, 1, C.c_void_p(out_), C.c_void_p(ws.data_ptr()), ws.numel() if wsb is None else wsb, 1, None)
    for fn in (lib.troyn_apply_galois_many, lib.troyn_apply_galois_sum):
        assert fn(*args()) == 0
        assert fn(*args(L_=0)) == -1
        assert fn(*args(el_=None)) == -1
        assert fn(*args(kp_=None)) == -1
        assert fn(*args(ct_=None)) == -1
        assert fn(*args(out_=None)) == -1
        assert fn(*args(out_=ct.data_ptr() + 16)) == -1
        assert fn(*args(wsb=ws.numel() - 8)) == -3
    torch.cuda.synchronize()
    # a smaller workspace is asked for the sum form than for the many form of the same call
    assert lib.troyn_apply_galois_hoisted_workspace_bytes(plan.h, L, 4, 2, 1) < lib.troyn_apply_galois_hoisted_workspace_bytes(plan.h, L, 4, 2, 0)
