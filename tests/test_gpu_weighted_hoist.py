"""Plaintext-weighted hoisted rotations on the GPU (troyn_apply_galois_weighted_sums) against the exact big-integer specification of
tests/weighted_hoist_spec.py -- never against another GPU path.

Small rings (N = 32 / 64): everything by definition.  N = 1024 .. 16384: the specification's negacyclic products and exact rounded division
on Python integers; only the NTT <-> coefficient form conversions of operands use the oracle's transform, which
tests/test_keyswitch_spec.py pins to the by-definition transform (as tests/test_gpu_hoist.py)."""
import ctypes as C

import numpy as np
import pytest

from ks_spec import negacyclic
from test_gpu_hoist import EDGE, _ints, _small_case
from test_keyswitch_spec import _ntt_polys
from weighted_hoist_spec import finish_weighted, keyed_inner_products

pytestmark = pytest.mark.gpu


def _keys_as_lists(keys_c):
    return [None if kt is None else [[_ints(kj[c]) for c in range(2)] for kj in kt] for kt in keys_c]


def _solve_weighted_boundary(q, L, c1, elements, keys_c, weights_s, rng):
    """test_gpu_hoist._solve_boundary after weighting: item data with digit 0 = the constant 1, term 0 keyed, present in the slot and weighted by
    the constant 1 on the special row.  Solves the special-prime rows of key (term 0, digit 0) so that the slot's WEIGHTED summed special-prime
    component sits on the rounding boundary at the first coefficients.  Returns P (keyed_inner_products) for the solved keys."""
    K, n = len(q), len(c1[0])
    qs, h = q[-1], q[-1] // 2
    assert [int(v) for v in c1[0][:2]] == [1, 0] and not any(int(v) for v in c1[0][1:])
    assert elements[0] != 1 and weights_s[0][K - 1] == [1] + [0] * (n - 1)
    for c in range(2):
        keys_c[0][0][c][K - 1][:] = 0
    P = keyed_inner_products(q, L, _ints(c1), elements, _keys_as_lists(keys_c))
    for c in range(2):
        target = [int(v) for v in rng.integers(0, qs, size=n, dtype=np.uint64)]
        edge = EDGE(qs, h)
        target[:len(edge)] = edge if c == 0 else edge[::-1]
        rest = [0] * n
        for t, w in enumerate(weights_s):
            if w is not None and elements[t] != 1:
                rest = [(x + y) % qs for x, y in zip(rest, negacyclic(w[K - 1], P[t][c][K - 1], qs))]
        row = [(x - y) % qs for x, y in zip(target, rest)]
        keys_c[0][0][c][K - 1][:] = np.array(row, dtype=np.uint64)
        # digit 0 of term 0 is the constant 1 and so is its weight on this row: the product with the solved row is the row itself
        P[0][c][K - 1] = [(x + y) % qs for x, y in zip(P[0][c][K - 1], row)]
    return P


def _random_weight(q, n, rng, unit_special=False):
    w = [[int(v) for v in rng.integers(0, m, size=n, dtype=np.uint64)] for m in q]
    if unit_special:
        w[-1] = [1] + [0] * (n - 1)
    return w


@pytest.mark.parametrize("n,bits,L,order", [(32, (50, 50, 50, 50), 3, None), (64, (60, 40, 40, 60), 3, None), (32, (50, 50, 50), 2, "reversed")])
@pytest.mark.parametrize("scheme,is_ntt", [("ckks", True), ("bfv", False)])
def test_small_rings_by_definition(O, pkg, dev, n, bits, L, order, scheme, is_ntt):
    """slots = 2: slot 0 = {5, 25, 2N - 1, identity}, slot 1 = {25} alone; random weights; two different items, item 0 on the rounding boundary
    of slot 0's weighted sum"""
    q, all_elements, items, all_keys, _ = _small_case(O, n, bits, L, order)
    elements = all_elements[:3] + [1]
    keys_c = [[kj.copy() for kj in all_keys[i]] for i in range(3)] + [None]
    rng = np.random.default_rng(n + 7 * L)
    weights = [[_random_weight(q, n, rng, unit_special=(t == 0)) for t in range(4)],
               [None, _random_weight(q, n, rng), None, None]]
    P0 = _solve_weighted_boundary(q, L, items[0][1], elements, keys_c, weights[0], rng)
    keys_l = _keys_as_lists(keys_c)
    assert P0 == keyed_inner_products(q, L, _ints(items[0][1]), elements, keys_l)
    P = [P0, keyed_inner_products(q, L, _ints(items[1][1]), elements, keys_l)]
    plan = pkg.Plan(dev, n.bit_length() - 1, q)
    dkeys = [None if kt is None else [pkg.to_device(np.stack([_ntt_polys(kj[c], q) for c in range(2)]), dev) for kj in kt] for kt in keys_c]
    dweights = [[None if w is None else pkg.to_device(_ntt_polys(np.array(w, dtype=np.uint64), q), dev) for w in row] for row in weights]
    form = (lambda x: np.stack([_ntt_polys(np.array(x[c], dtype=np.uint64), q[:L]) for c in range(2)])) if is_ntt else (lambda x: np.array(x, dtype=np.uint64))
    ct = pkg.to_device(np.stack([form(np.stack(it)) for it in items]), dev)
    got = pkg.to_host(plan.apply_galois_weighted_sums(L, ct, elements, dkeys, dweights, is_ckks=(scheme == "ckks"), is_ntt_form=is_ntt))
    assert got.shape == (2, 2, 2, L, n)
    for s in range(2):
        for b in range(2):
            want = finish_weighted(q, L, _ints(items[b][0]), _ints(items[b][1]), elements, P[b], weights[s])
            assert np.array_equal(got[s, b], form(want)), (s, b)


@pytest.mark.parametrize("n,bits,L,is_ntt", [(8192, [40, 40, 40], 2, False),
                                             (8192, [60, 40, 40, 60], 3, True),
                                             (16384, [50] * 6, 5, True)])
def test_kernel_sizes_against_spec(O, pkg, dev, n, bits, L, is_ntt):
    """batch = 8 identical items (groups of four items per workgroup, two groups), elements {5, 2N - 1, identity}, one slot; the weighted summed
    special-prime component on the rounding boundary"""
    q = [int(v) for v in O.coeff_modulus_create(n, bits)]
    K = len(q)
    plan = pkg.Plan(dev, n.bit_length() - 1, q)
    rng = np.random.default_rng(79)
    elements = [5, 2 * n - 1, 1]
    c0 = np.stack([rng.integers(0, q[l], size=n, dtype=np.uint64) for l in range(L)])
    c1 = np.stack([rng.integers(0, q[l], size=n, dtype=np.uint64) for l in range(L)])
    c1[0] = 0
    c1[0, 0] = 1
    keys_c = [[np.stack([np.stack([rng.integers(0, q[k], size=n, dtype=np.uint64) for k in range(K)]) for c in range(2)]) for j in range(L)] for t in range(2)] + [None]
    weights = [_random_weight(q, n, rng, unit_special=(t == 0)) for t in range(3)]
    P = _solve_weighted_boundary(q, L, c1, elements, keys_c, weights, rng)

    def to_ntt_rows(x, rows):        # x [len(rows)][N] under moduli q[rows]; the oracle's transform, conversions only
        out = np.empty_like(x)
        for i, r in enumerate(rows):
            c1x = O.Context("ckks", n, [q[r], q[(r + 1) % K]])
            out[i] = c1x.to_ntt(x[i][None, None], 1, 1)[0, 0]
        return out

    data = list(range(L))
    form = (lambda x: np.stack([to_ntt_rows(np.array(x[c], dtype=np.uint64), data) for c in range(2)])) if is_ntt else (lambda x: np.array(x, dtype=np.uint64))
    dkeys = [None if kt is None else [pkg.to_device(np.stack([to_ntt_rows(kj[c], list(range(K))) for c in range(2)]), dev) for kj in kt] for kt in keys_c]
    dweights = [[pkg.to_device(to_ntt_rows(np.array(w, dtype=np.uint64), list(range(K))), dev) for w in weights]]
    batch = 8
    ct = pkg.to_device(np.repeat(form(np.stack([c0, c1]))[None], batch, axis=0), dev)
    got = pkg.to_host(plan.apply_galois_weighted_sums(L, ct, elements, dkeys, dweights, is_ckks=is_ntt, is_ntt_form=is_ntt))
    assert got.shape == (1, batch, 2, L, n)
    want = form(finish_weighted(q, L, _ints(c0), _ints(c1), elements, P, weights))
    for i in (0, 3, 7):
        assert np.array_equal(got[0, i], want), i


def test_accumulator_range(O, pkg, dev):
    """22 terms x 3 digits, every digit q_j - 1, every key word m - 1 and every weight word m - 1 (one key and one weight buffer shared by all
    terms): the accumulator is reduced once per term, weighted, and never runs across terms"""
    n, L, terms = 1024, 3, 22
    q = [int(v) for v in O.coeff_modulus_create(n, [60, 60, 60, 60])]
    K = len(q)
    plan = pkg.Plan(dev, 10, q)
    elements = [3 + 2 * t for t in range(terms)]
    const_ntt = np.stack([np.full(n, q[k] - 1, dtype=np.uint64) for k in range(K)])
    # the transform of a constant polynomial is that constant at every point: in coefficient form it is (m - 1) at X^0
    const_c = [[q[k] - 1] + [0] * (n - 1) for k in range(K)]
    rng = np.random.default_rng(9)
    c0 = np.stack([rng.integers(0, q[l], size=n, dtype=np.uint64) for l in range(L)])
    c1 = np.stack([np.full(n, q[l] - 1, dtype=np.uint64) for l in range(L)])
    P = keyed_inner_products(q, L, _ints(c1), elements, [[[const_c, const_c]] * L] * terms)
    dkey = pkg.to_device(np.stack([const_ntt, const_ntt]), dev)
    dweight = pkg.to_device(const_ntt, dev)
    ct = pkg.to_device(np.stack([c0, c1])[None], dev)
    got = pkg.to_host(plan.apply_galois_weighted_sums(L, ct, elements, [[dkey] * L] * terms, [[dweight] * terms], is_ckks=False, is_ntt_form=False))
    want = finish_weighted(q, L, _ints(c0), _ints(c1), elements, P, [const_c] * terms)
    assert np.array_equal(got[0, 0], np.array(want, dtype=np.uint64))


@pytest.mark.parametrize("batch", [1, 2, 3, 5])
@pytest.mark.parametrize("is_ntt", [True, False])
def test_batch_grouping(O, pkg, dev, batch, is_ntt):
    """one, two and four items per workgroup, with a padded last group (batch = 3: 2 + 1, batch = 5: 4 + 1)"""
    n, L = 64, 3
    q, all_elements, items, all_keys, _ = _small_case(O, n, (60, 40, 40, 60), L, None)
    elements = [1, all_elements[0], all_elements[2]]
    keys_c = [None, all_keys[0], all_keys[2]]
    rng = np.random.default_rng(batch)
    weights = [_random_weight(q, n, rng) for _ in elements]
    keys_l = _keys_as_lists(keys_c)
    plan = pkg.Plan(dev, 6, q)
    dkeys = [None if kt is None else [pkg.to_device(np.stack([_ntt_polys(kj[c], q) for c in range(2)]), dev) for kj in kt] for kt in keys_c]
    dweights = [[pkg.to_device(_ntt_polys(np.array(w, dtype=np.uint64), q), dev) for w in weights]]
    form = (lambda x: np.stack([_ntt_polys(np.array(x[c], dtype=np.uint64), q[:L]) for c in range(2)])) if is_ntt else (lambda x: np.array(x, dtype=np.uint64))
    want = [form(finish_weighted(q, L, _ints(it[0]), _ints(it[1]), elements, keyed_inner_products(q, L, _ints(it[1]), elements, keys_l), weights)) for it in items]
    ct = pkg.to_device(np.stack([form(np.stack(items[b % 2])) for b in range(batch)]), dev)
    got = pkg.to_host(plan.apply_galois_weighted_sums(L, ct, elements, dkeys, dweights, is_ckks=is_ntt, is_ntt_form=is_ntt))
    assert got.shape == (1, batch, 2, L, n)
    for b in range(batch):
        assert np.array_equal(got[0, b], want[b % 2]), b


def test_errors(O, pkg, dev):
    import torch
    n, L = 32, 2
    q = O.coeff_modulus_create(n, [40, 40, 40])
    K = len(q)
    plan = pkg.Plan(dev, 5, q)
    lib = pkg.capi.lib()
    ctx = O.Context("ckks", n, q)
    ct = pkg.to_device(ctx.random_ct(1, 2, L)[None], dev)
    key = [pkg.to_device(k, dev) for k in ctx.random_keys(2, L)]
    w = pkg.to_device(np.ones((K, n), dtype=np.uint64), dev)
    INVALID = pkg.capi.TroynInvalidArgument
    fn = plan.apply_galois_weighted_sums
    with pytest.raises(INVALID):
        fn(L, ct, [], [], [[]])                                     # terms == 0
    with pytest.raises(INVALID):
        fn(L, ct, [3], [key], [])                                   # slots == 0
    with pytest.raises(INVALID):
        fn(L, ct, [3, 5], [key, key], [[w, w], [None, None]])       # a slot with no weight
    for bad in (4, 2 * n, 2 * n + 1):                               # even, >= 2N
        with pytest.raises(INVALID):
            fn(L, ct, [3, bad], [key, key], [[w, w]])
    with pytest.raises(INVALID):
        fn(L, ct, [3], [[key[0], None]], [[w]])                     # a null key entry of a term with g != 1
    with pytest.raises(INVALID):
        fn(3, pkg.to_device(np.zeros((1, 2, 3, n), dtype=np.uint64), dev), [3], [key + key], [[w]])      # L = K
    with pytest.raises(INVALID):
        fn(L, ct, [3], [key], [[w]], out=ct)                        # out overlapping ct
    assert fn(L, ct[:0], [3], [key], [[w]]).numel() == 0            # batch == 0: TROYN_OK, nothing launched
    # the identity needs no key: its entry may be None, or hold nulls
    a = pkg.to_host(fn(L, ct, [1, 3], [None, key], [[w, w]]))
    b = pkg.to_host(fn(L, ct, [1, 3], [[None] * L, key], [[w, w]]))
    assert np.array_equal(a, b)
    # the raw entry: null tables, L = 0, misaligned pointers, a short workspace, a NULL key entry on an identity term
    ws = torch.empty(lib.troyn_apply_galois_weighted_workspace_bytes(plan.h, L, 2, 1, 1, 1), dtype=torch.uint8, device=dev)
    out = torch.empty_like(ct)
    el = (C.c_uint64 * 2)(3, 1)
    kp = (C.c_void_p * (2 * L))(*([k.data_ptr() for k in key] + [None] * L))
    wp = (C.c_void_p * 2)(w.data_ptr(), w.data_ptr())
    raw = lib.troyn_apply_galois_weighted_sums
    args = lambda L_=L, ct_=ct.data_ptr(), el_=el, kp_=kp, wp_=wp, out_=out.data_ptr(), ws_=ws.data_ptr(), wsb=None, terms=2, slots=1: (
        plan.h, L_, 1, 1, C.c_void_p(ct_), el_, kp_, terms, wp_, slots, C.c_void_p(out_), C.c_void_p(ws_), ws.numel() if wsb is None else wsb, 1, None)
    assert raw(*args()) == 0                                        # NULL key entries on the identity term are accepted
    assert raw(*args(L_=0)) == -1
    assert raw(*args(terms=0)) == -1
    assert raw(*args(slots=0)) == -1
    assert raw(*args(el_=None)) == -1
    assert raw(*args(kp_=None)) == -1
    assert raw(*args(wp_=None)) == -1
    assert raw(*args(ct_=None)) == -1
    assert raw(*args(out_=None)) == -1
    assert raw(*args(ct_=ct.data_ptr() + 8)) == -1
    assert raw(*args(out_=out.data_ptr() + 8)) == -1
    assert raw(*args(ws_=ws.data_ptr() + 8)) == -1
    assert raw(*args(out_=ct.data_ptr() + 16)) == -1
    assert raw(*args(kp_=(C.c_void_p * (2 * L))(key[0].data_ptr() + 8, key[1].data_ptr(), None, None))) == -1
    assert raw(*args(kp_=(C.c_void_p * (2 * L))(None, key[1].data_ptr(), None, None))) == -1
    assert raw(*args(wp_=(C.c_void_p * 2)(w.data_ptr() + 8, w.data_ptr()))) == -1
    assert raw(*args(wp_=(C.c_void_p * 2)(None, None))) == -1
    assert raw(*args(el_=(C.c_uint64 * 2)(3, 2 * n))) == -1
    assert raw(*args(wsb=ws.numel() - 8)) == -3
    torch.cuda.synchronize()
    # the coefficient form asks for room for the transformed c0 on top
    wb = lib.troyn_apply_galois_weighted_workspace_bytes
    assert wb(plan.h, L, 2, 1, 1, 0) == wb(plan.h, L, 2, 1, 1, 1) + L * n * 8
