"""The sum of key-switched automorphisms of DIFFERENT ciphertexts on the GPU (troyn_apply_galois_sum_each) against the exact big-integer
specification of tests/bsgs_spec.py -- never against another GPU path, except for the one cross-check with troyn_apply_galois_sum (itself
pinned to its specification by tests/test_gpu_hoist.py).

Small rings (N = 32 / 64): everything by definition.  N = 1024 .. 16384: the specification's negacyclic products and exact rounded division
on Python integers; only the NTT <-> coefficient form conversions of operands use the oracle's transform, which
tests/test_keyswitch_spec.py pins to the by-definition transform (as tests/test_gpu_hoist.py)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from bsgs_spec import each_inner_products, sum_each_spec
from test_gpu_hoist import EDGE, _ints, _small_case
from test_gpu_weighted_hoist import _keys_as_lists
from test_keyswitch_spec import _ntt_polys

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GROUP = int(re.search(r"^#define TROYN_HOIST_EACH_GROUP (\d+)$", open(os.path.join(ROOT, "include", "troyn.h")).read(), flags=re.M).group(1))


def _random_ct(q, L, n, rng, unit_digit=False):
    c0 = np.stack([rng.integers(0, q[l], size=n, dtype=np.uint64) for l in range(L)])
    c1 = np.stack([rng.integers(0, q[l], size=n, dtype=np.uint64) for l in range(L)])
    if unit_digit:
        c1[0] = 0
        c1[0, 0] = 1
    return c0, c1


def _as_lists(cts):
    return [(_ints(c0), _ints(c1)) for c0, c1 in cts]


def _solve_each_boundary(q, L, cts, elements, keys_c, rng):
    """test_gpu_hoist._solve_boundary over different ciphertexts: digit 0 of term 0 is the constant 1 and term 0 is keyed.  Solves the
    special-prime rows of key (term 0, digit 0) so that the special-prime component SUMMED over the terms sits on the rounding boundary at the
    first coefficients.  Returns P (each_inner_products) for the solved keys."""
    K, n = len(q), len(cts[0][1][0])
    qs, h = q[-1], q[-1] // 2
    c1 = cts[0][1]
    assert elements[0] != 1 and [int(v) for v in c1[0][:2]] == [1, 0] and not any(int(v) for v in c1[0][1:])
    for c in range(2):
        keys_c[0][0][c][K - 1][:] = 0
    P = each_inner_products(q, L, _as_lists(cts), elements, _keys_as_lists(keys_c))
    for c in range(2):
        target = [int(v) for v in rng.integers(0, qs, size=n, dtype=np.uint64)]
        edge = EDGE(qs, h)
        target[:len(edge)] = edge if c == 0 else edge[::-1]
        rest = [0] * n
        for t, g in enumerate(elements):
            if g != 1:
                rest = [(x + y) % qs for x, y in zip(rest, P[t][c][K - 1])]
        row = [(x - y) % qs for x, y in zip(target, rest)]
        keys_c[0][0][c][K - 1][:] = np.array(row, dtype=np.uint64)
        # digit 0 of term 0 is the constant 1: its product with the solved row is the row itself
        P[0][c][K - 1] = [(x + y) % qs for x, y in zip(P[0][c][K - 1], row)]
    return P


def _small_forms(q, L, is_ntt):
    if is_ntt:
        return lambda x: np.stack([_ntt_polys(np.array(x[c], dtype=np.uint64), q[:L]) for c in range(2)])
    return lambda x: np.array(x, dtype=np.uint64)


def _small_keys(pkg, dev, q, keys_c):
    return [None if kt is None else [pkg.to_device(np.stack([_ntt_polys(kj[c], q) for c in range(2)]), dev) for kj in kt] for kt in keys_c]


@pytest.mark.parametrize("n,bits,L,order", [(32, (50, 50, 50, 50), 3, None), (64, (60, 40, 40, 60), 3, None), (32, (50, 50, 50), 2, "reversed")])
@pytest.mark.parametrize("scheme,is_ntt", [("ckks", True), ("bfv", False)])
def test_small_rings_by_definition(O, pkg, dev, n, bits, L, order, scheme, is_ntt):
    """terms {5, 25, 2N - 1, identity} over four DIFFERENT ciphertexts, two different items, item 0 on the rounding boundary of the sum"""
    q, all_elements, _, all_keys, _ = _small_case(O, n, bits, L, order)
    elements = all_elements[:3] + [1]
    keys_c = [[kj.copy() for kj in all_keys[i]] for i in range(3)] + [None]
    rng = np.random.default_rng(3 * n + L)
    items = [[_random_ct(q, L, n, rng, unit_digit=(b == 0 and t == 0)) for t in range(4)] for b in range(2)]
    P0 = _solve_each_boundary(q, L, items[0], elements, keys_c, rng)
    keys_l = _keys_as_lists(keys_c)
    assert P0 == each_inner_products(q, L, _as_lists(items[0]), elements, keys_l)
    plan = pkg.Plan(dev, n.bit_length() - 1, q)
    form = _small_forms(q, L, is_ntt)
    cts = pkg.to_device(np.stack([np.stack([form(np.stack(items[b][t])) for b in range(2)]) for t in range(4)]), dev)
    got = pkg.to_host(plan.apply_galois_sum_each(L, cts, elements, _small_keys(pkg, dev, q, keys_c), is_ckks=(scheme == "ckks"), is_ntt_form=is_ntt))
    assert got.shape == (2, 2, L, n)
    for b in range(2):
        want = sum_each_spec(q, L, _as_lists(items[b]), elements, keys_l, P=P0 if b == 0 else None)
        assert np.array_equal(got[b], form(want)), b


@pytest.mark.parametrize("n,bits,L,is_ntt", [(8192, [40, 40, 40], 2, False),
                                             (8192, [60, 40, 40, 60], 3, True),
                                             (16384, [50] * 6, 5, True)])
def test_kernel_sizes_against_spec(O, pkg, dev, n, bits, L, is_ntt):
    """batch = 5 identical items (a group of four items per workgroup and a padded one), three different ciphertexts under {5, 2N - 1, identity};
    the summed special-prime component on the rounding boundary"""
    q = [int(v) for v in O.coeff_modulus_create(n, bits)]
    K = len(q)
    plan = pkg.Plan(dev, n.bit_length() - 1, q)
    rng = np.random.default_rng(83)
    elements = [5, 2 * n - 1, 1]
    cts = [_random_ct(q, L, n, rng, unit_digit=(t == 0)) for t in range(3)]
    keys_c = [[np.stack([np.stack([rng.integers(0, q[k], size=n, dtype=np.uint64) for k in range(K)]) for c in range(2)]) for j in range(L)] for t in range(2)] + [None]
    P = _solve_each_boundary(q, L, cts, elements, keys_c, rng)

    def to_ntt_rows(x, rows):        # x [len(rows)][N] under moduli q[rows]; the oracle's transform, conversions only
        out = np.empty_like(x)
        for i, r in enumerate(rows):
            c1x = O.Context("ckks", n, [q[r], q[(r + 1) % K]])
            out[i] = c1x.to_ntt(x[i][None, None], 1, 1)[0, 0]
        return out

    data = list(range(L))
    form = (lambda x: np.stack([to_ntt_rows(np.array(x[c], dtype=np.uint64), data) for c in range(2)])) if is_ntt else (lambda x: np.array(x, dtype=np.uint64))
    dkeys = [None if kt is None else [pkg.to_device(np.stack([to_ntt_rows(kj[c], list(range(K))) for c in range(2)]), dev) for kj in kt] for kt in keys_c]
    batch = 5
    dcts = pkg.to_device(np.stack([np.repeat(form(np.stack(ct))[None], batch, axis=0) for ct in cts]), dev)
    got = pkg.to_host(plan.apply_galois_sum_each(L, dcts, elements, dkeys, is_ckks=is_ntt, is_ntt_form=is_ntt))
    assert got.shape == (batch, 2, L, n)
    want = form(sum_each_spec(q, L, _as_lists(cts), elements, None, P=P))
    for i in (0, 3, 4):
        assert np.array_equal(got[i], want), i


@pytest.mark.parametrize("is_ntt", [True, False])
def test_term_grouping(O, pkg, dev, is_ntt):
    """2 * TROYN_HOIST_EACH_GROUP + 1 terms, each a different ciphertext: two full groups and a last group of one; the words are the
    specification's whatever the grouping, and the workspace is that of one group"""
    n, L = 64, 3
    q, all_elements, _, all_keys, _ = _small_case(O, n, (60, 40, 40, 60), L, None)
    terms = 2 * GROUP + 1
    pick = [t % 5 for t in range(terms)]                       # the four keyed elements and the identity in turn
    elements = [1 if i == 4 else all_elements[i] for i in pick]
    keys_c = [None if i == 4 else all_keys[i] for i in pick]
    rng = np.random.default_rng(terms)
    cts = [_random_ct(q, L, n, rng) for _ in range(terms)]
    plan = pkg.Plan(dev, 6, q)
    form = _small_forms(q, L, is_ntt)
    shared = _small_keys(pkg, dev, q, list(all_keys))
    dkeys = [None if i == 4 else shared[i] for i in pick]
    dcts = pkg.to_device(np.stack([form(np.stack(ct))[None] for ct in cts]), dev)
    got = pkg.to_host(plan.apply_galois_sum_each(L, dcts, elements, dkeys, is_ckks=is_ntt, is_ntt_form=is_ntt))
    want = sum_each_spec(q, L, _as_lists(cts), elements, _keys_as_lists(keys_c))
    assert np.array_equal(got[0], form(want))
    wb = pkg.capi.lib().troyn_apply_galois_sum_each_workspace_bytes
    for batch in (1, 5):
        assert wb(plan.h, L, terms, batch, int(is_ntt)) == wb(plan.h, L, GROUP, batch, int(is_ntt))
        assert wb(plan.h, L, GROUP - 1, batch, int(is_ntt)) < wb(plan.h, L, GROUP, batch, int(is_ntt))


def test_accumulator_range(O, pkg, dev):
    """22 terms x 3 digits, every digit q_j - 1 and every key word m - 1 (one key buffer shared by all terms): the accumulator is reduced once
    per term and never runs across terms, nor across the groups of terms"""
    n, L, terms = 1024, 3, 22
    q = [int(v) for v in O.coeff_modulus_create(n, [60, 60, 60, 60])]
    K = len(q)
    plan = pkg.Plan(dev, 10, q)
    elements = [3 + 2 * t for t in range(terms)]
    const_ntt = np.stack([np.full(n, q[k] - 1, dtype=np.uint64) for k in range(K)])
    # the transform of a constant polynomial is that constant at every point: in coefficient form it is (m - 1) at X^0
    const_c = [[q[k] - 1] + [0] * (n - 1) for k in range(K)]
    rng = np.random.default_rng(10)
    c1 = np.stack([np.full(n, q[l] - 1, dtype=np.uint64) for l in range(L)])
    cts = [(np.stack([rng.integers(0, q[l], size=n, dtype=np.uint64) for l in range(L)]), c1) for _ in range(terms)]
    dkey = pkg.to_device(np.stack([const_ntt, const_ntt]), dev)
    dcts = pkg.to_device(np.stack([np.stack(ct)[None] for ct in cts]), dev)
    got = pkg.to_host(plan.apply_galois_sum_each(L, dcts, elements, [[dkey] * L] * terms, is_ckks=False, is_ntt_form=False))
    want = sum_each_spec(q, L, _as_lists(cts), elements, [[[const_c, const_c]] * L] * terms)
    assert np.array_equal(got[0], np.array(want, dtype=np.uint64))


@pytest.mark.parametrize("batch", [1, 2, 3, 5])
@pytest.mark.parametrize("is_ntt", [True, False])
def test_batch_grouping(O, pkg, dev, batch, is_ntt):
    """one, two and four items per workgroup, with a padded last group (batch = 3: 2 + 1, batch = 5: 4 + 1); every item different"""
    n, L = 64, 3
    q, all_elements, _, all_keys, _ = _small_case(O, n, (60, 40, 40, 60), L, None)
    elements = [1, all_elements[0], all_elements[2]]
    keys_c = [None, all_keys[0], all_keys[2]]
    keys_l = _keys_as_lists(keys_c)
    rng = np.random.default_rng(40 + batch)
    items = [[_random_ct(q, L, n, rng) for _ in elements] for _ in range(batch)]
    plan = pkg.Plan(dev, 6, q)
    form = _small_forms(q, L, is_ntt)
    dcts = pkg.to_device(np.stack([np.stack([form(np.stack(items[b][t])) for b in range(batch)]) for t in range(3)]), dev)
    got = pkg.to_host(plan.apply_galois_sum_each(L, dcts, elements, _small_keys(pkg, dev, q, keys_c), is_ckks=is_ntt, is_ntt_form=is_ntt))
    assert got.shape == (batch, 2, L, n)
    for b in range(batch):
        assert np.array_equal(got[b], form(sum_each_spec(q, L, _as_lists(items[b]), elements, keys_l))), b


@pytest.mark.parametrize("n,bits,L,scheme,is_ntt", [(64, [60, 40, 40, 60], 3, "ckks", True), (64, [60, 40, 40, 60], 3, "bfv", False),
                                                    (8192, [60, 40, 40, 60], 3, "ckks", True), (8192, [40, 40, 40], 2, "bfv", False)])
def test_equal_terms_are_the_summed_form(O, pkg, dev, n, bits, L, scheme, is_ntt):
    """the cross-check: every term the same ciphertext and no identity term gives troyn_apply_galois_sum's words"""
    q = O.coeff_modulus_create(n, bits)
    plan = pkg.Plan(dev, n.bit_length() - 1, q)
    ctx = O.Context("ckks", n, q)
    batch, elements = 3, [5, 25, 2 * n - 1]
    ct = pkg.to_device(np.stack([ctx.random_ct(50 + b, 2, L) for b in range(batch)]), dev)
    keys = [[pkg.to_device(k, dev) for k in ctx.random_keys(60 + t, L)] for t in range(3)]
    want = pkg.to_host(plan.apply_galois_sum(L, ct, elements, keys, is_ckks=(scheme == "ckks"), is_ntt_form=is_ntt))
    cts = ct[None].repeat(3, 1, 1, 1, 1).contiguous()
    got = pkg.to_host(plan.apply_galois_sum_each(L, cts, elements, keys, is_ckks=(scheme == "ckks"), is_ntt_form=is_ntt))
    assert np.array_equal(got, want)


def test_errors(O, pkg, dev):
    import torch
    n, L = 32, 2
    q = O.coeff_modulus_create(n, [40, 40, 40])
    plan = pkg.Plan(dev, 5, q)
    lib = pkg.capi.lib()
    ctx = O.Context("ckks", n, q)
    cts = pkg.to_device(np.stack([ctx.random_ct(1 + t, 2, L)[None] for t in range(2)]), dev)      # [2][1][2][L][N]
    key = [pkg.to_device(k, dev) for k in ctx.random_keys(2, L)]
    INVALID = pkg.capi.TroynInvalidArgument
    fn = plan.apply_galois_sum_each
    with pytest.raises(INVALID):
        fn(L, cts, [], [])                                           # terms == 0
    for bad in (4, 2 * n, 2 * n + 1):                                # even, >= 2N
        with pytest.raises(INVALID):
            fn(L, cts, [3, bad], [key, key])
    with pytest.raises(INVALID):
        fn(L, cts, [3, 5], [key, [key[0], None]])                    # a null key entry of a keyed term
    with pytest.raises(INVALID):
        fn(3, pkg.to_device(np.zeros((2, 1, 2, 3, n), dtype=np.uint64), dev), [3, 5], [key + key, key + key])      # L = K
    with pytest.raises(INVALID):
        fn(L, cts, [3, 5], [key, key], out=cts[1])                   # out overlapping cts
    assert fn(L, cts[:, :0], [3, 5], [key, key]).numel() == 0       # batch == 0: TROYN_OK, nothing launched
    # the identity needs no key: its entry may be None, or hold nulls
    a = pkg.to_host(fn(L, cts, [1, 3], [None, key]))
    b = pkg.to_host(fn(L, cts, [1, 3], [[None] * L, key]))
    assert np.array_equal(a, b)
    # the raw entry: null tables, L = 0, misaligned pointers, a short workspace, overlap, batch == 0, NULL keys on an identity term
    wb = lib.troyn_apply_galois_sum_each_workspace_bytes
    ws = torch.empty(wb(plan.h, L, 2, 1, 1), dtype=torch.uint8, device=dev)
    out = torch.empty_like(cts[0])
    el = (C.c_uint64 * 2)(3, 1)
    kp = (C.c_void_p * (2 * L))(*([k.data_ptr() for k in key] + [None] * L))
    raw = lib.troyn_apply_galois_sum_each
    args = lambda L_=L, ct_=cts.data_ptr(), el_=el, kp_=kp, out_=out.data_ptr(), ws_=ws.data_ptr(), wsb=None, terms=2, batch=1: (
        plan.h, L_, 1, 1, C.c_void_p(ct_), el_, kp_, terms, C.c_void_p(out_), C.c_void_p(ws_), ws.numel() if wsb is None else wsb, batch, None)
    assert raw(*args()) == 0                                         # NULL key entries on the identity term are accepted
    assert raw(*args(L_=0)) == -1
    assert raw(*args(terms=0)) == -1
    assert raw(*args(el_=None)) == -1
    assert raw(*args(kp_=None)) == -1
    assert raw(*args(ct_=None)) == -1
    assert raw(*args(out_=None)) == -1
    assert raw(*args(ws_=None)) == -1
    assert raw(*args(ct_=cts.data_ptr() + 8)) == -1
    assert raw(*args(out_=out.data_ptr() + 8)) == -1
    assert raw(*args(ws_=ws.data_ptr() + 8)) == -1
    assert raw(*args(out_=cts.data_ptr() + 16)) == -1                # overlaps term 0
    assert raw(*args(out_=cts[1].data_ptr())) == -1                  # overlaps the last term
    assert raw(*args(kp_=(C.c_void_p * (2 * L))(key[0].data_ptr() + 8, key[1].data_ptr(), None, None))) == -1
    assert raw(*args(kp_=(C.c_void_p * (2 * L))(None, key[1].data_ptr(), None, None))) == -1
    assert raw(*args(el_=(C.c_uint64 * 2)(3, 2 * n))) == -1
    assert raw(*args(el_=(C.c_uint64 * 2)(3, 4))) == -1
    assert raw(*args(wsb=ws.numel() - 8)) == -3
    assert raw(*args(batch=0, ct_=None, out_=None, ws_=None, wsb=0)) == 0
    torch.cuda.synchronize()
    # the coefficient form asks for room for the transformed c0 of the resident terms on top
    assert wb(plan.h, L, 2, 1, 0) == wb(plan.h, L, 2, 1, 1) + 2 * L * n * 8
